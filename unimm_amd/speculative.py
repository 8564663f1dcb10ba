"""Speculative answer generation: a draft model proposes, the model verifies (`generate_answers(draft=..., draft_len=g)`): greedy
decoding first, speculative SAMPLING at the end.

The answers are those of the plain beams = 1 call (up to the batch dependence of the logits, the caveat of `generation.py`): the
draft only decides how many of them one pass of the model yields.  The mask argument of `generation.py` is what makes it exact:
answer row k depends on earlier answer rows only and copy row k on the context and the answer rows before k, so the g + 1 pairs
(answer row n-1+j, copy row n+j), j = 0 .. g, can go through the model's blocks at once, provided each new row attends the answer
rows of the pairs up to its own, itself if it is a copy row, and no other new row -- `unimm_attn_verify` (include/unimm_hip.h).

State per slot (one slot per dialog): n[s] tokens emitted so far, a finished flag, the output tables.  Token 0 comes from the
model's prefill row, as in the plain call; the draft is prefilled once too, for its context and region caches (its prefill
logits are not used).  One round, for every live slot:

1. DRAFT.  The draft decodes g greedy tokens d_0 .. d_{g-1} for steps n .. n + g - 1 with its own decode steps (`unimm_lm_topk`,
   K = 1) under the step rules of the step each row stands at: the banned ids, [SEP] banned while the step is below
   min_answer_len, [SEP] forced once the step reaches the dialog's limit.  Steps are per slot: flags and position ids come from
   n[s] + j.
2. VERIFY.  The model pushes the g + 1 pairs of every slot through its blocks in one pass: answer row n-1 holds the last emitted
   token, answer rows n .. n+g-1 the drafts.  One `unimm_lm_topk` launch (K = 1, per-row flags of step n + j) on the g + 1 copy
   rows gives the model's own tokens t_0 .. t_g and their log p.
3. ACCEPT.  a[s] = the number of leading j with d_j == t_j, stopping after an accepted [SEP].  The slot emits t_0 .. t_a -- the
   a accepted drafts and the model's own next token, each with the MODEL's log p -- cut after the first [SEP] among them, which
   finishes the slot.  A slot never emits past its limit: the forced [SEP] sees to it.  torch ops on [S, g + 1]; the round's one
   device -> host synchronisation is the "all slots finished" flag.
4. COMMIT.  The K | V of the answer rows of the tokens the model kept (rows n-1 .. n-1+a) join its private cache in place
   (`unimm_kv_cache_append`, a count per slot); the draft's cache rolls back to the rows of kept tokens, an assignment to its plen.

The fully accepted round (a = g) leaves the draft without the cached row of d_{g-1}: the draft never pushed that token.  Closed
uniformly: from round 2 on the draft's plen is set to n - 2 and its FIRST step of the round pushes two pairs per slot, for answer
rows n-2 and n-1 (through `unimm_attn_verify`, nr = 4), and appends both rows.  Row n-2 is recomputed where it was not missing
(the same values: a row's K | V depend on the tokens before it only).  Round 1 (n = 1) pushes the one pair of a plain decode step.

Caches: the model's holds pcap >= the largest limit rows per slot, the draft's the largest limit + g (what it appends before a
rollback).  Rows a finished slot or a step past a dialog's limit still pushes are computed and dropped; their position ids stop
at the limit's, and every cache index is clamped by the kernels.

`speculative_search` is written against abstract step functions, as `beam_search` is (the CPU tests drive it with table models);
`speculate` supplies the engines': two sides of `decoding.py`, the model's and the draft's.

Speculative SAMPLING (`generate_answers(samples=N, draft=..., draft_accept="rejection")`, `speculative_sample_search`).  The same
rounds with one slot per (dialog, draw) -- S = G * N slots, plus one greedy slot per dialog with greedy=True -- and the standard
rejection rule in place of the comparison of tokens, so that the answers are distributed EXACTLY as the plain sampling call's:

1. DRAFT.  The draft DRAWS d_j from its own filtered distribution Q~ (`unimm_lm_sample_rows` with the slot's temperature / top_k /
   top_p, the model's, and the step rules of step n + j) and keeps the logits row it drew from.
2. VERIFY.  After the model's one pass, ONE `unimm_lm_spec_verify` launch on the S (g + 1) copy rows: row j < g accepts d_j with
   probability min(1, P~(d_j) / Q~(d_j)) and otherwise draws from the normalised residual max(0, P~ - Q~); row g (no draft) is a
   plain draw from P~, the bonus token after a fully accepted round.  P~ is the distribution the plain call samples from.
3. ACCEPT.  The match mask is the kernel's `accept`, the emitted tokens are its `token` at positions 0 .. a (the a accepted drafts,
   then the residual or bonus draw), each with the model's log p (step_logp) and log P~ (step_logq: the token of an
   accept-or-residual step is distributed as P~, which is what `PolicyObjective(mode="ratio")` needs).  The cut after an accepted
   [SEP], the counters, the flags and the one synchronisation per round are the greedy loop's (`_rounds` is both).
4. COMMIT as above.

Slots and groups.  `unimm_attn_verify` takes beams * nr <= 32 query rows per group, so every slot is a group of its own
(`decoding.DecodeSide` with per_group = 1): draft_len <= 15 holds for any samples <= 16, and no attention kernel changes.

Noise.  Token k of slot s is decided by three independent words per id: the draft's Gumbel noise, the accept uniform and the
residual's Gumbel noise, keyed by dropout.make_key(seed, k, site) with site = DRAFT_SITE / ACCEPT_SITE / RESIDUAL_SITE and the
stream of the plain sampling call (sample_streams[g] * N + j) -- k is the ABSOLUTE step of the token, not the round.  That stays
exact: a draft of step k + 1 that is discarded was discarded because of decisions at steps <= k, which read the noise of steps <= k
only; the noise of step k + 1 is independent of them, so when step k + 1 is drafted again after another prefix it is fresh for
that prefix.  A seed fixes the answers for a GIVEN draft_len only: which steps are drafted rows and which the bonus row, a plain
draw, depends on draft_len, so another draft_len gives other draws of the same distribution.  A launch carries one key, and the
rows of a launch stand at different steps; since make_key is site_key ^ step_salt and the sampler hashes key ^ affine(stream),
`step_streams` moves the step's salt into the stream id, and one launch keyed by site_key draws for every row what a launch keyed
by its own step would.
Token 0 and the bonus token are plain draws keyed by RESIDUAL_SITE (a row without a draft is `unimm_lm_sample_rows`, bit for bit).
A greedy slot is a top_k = 1 row on both sides: the draft's first id, accept = (draft == the model's first id), log q = 0.

Memory.  The draft's logits rows of a round stay alive until the verify launch: fp32 [S, draft_len + 1, Vpad] (row draft_len of
every slot is the bonus row's placeholder and never read), next to the model's own [S (draft_len + 1), Vpad] -- 80 dialogs x 8
samples at draft_len 4 and Vpad 30528: 391 MB each.
"""
from __future__ import annotations

import zlib
from collections import namedtuple

import numpy as np
import torch

from . import lib as L
from .decoding import DecodeSide
from .generation import (F32, SEP, GeneratedAnswers, Speculation, _greedy_sums, check_model, row_flags, sampled_answers)
from .lib import attn_verify, kv_cache_append, lm_spec_verify  # noqa: F401  (the names they had here before they joined lib.py)

DRAFT_SITE, ACCEPT_SITE, RESIDUAL_SITE = (zlib.crc32(b) & 0xFFFFFFFF for b in (b"generate.spec.draft", b"generate.spec.accept",
                                                                           b"generate.spec.residual"))   # as SAMPLE_SITE
MAX_DRAFT_LEN = 15                               # 2 * (draft_len + 1) <= 32 query rows per slot (unimm_attn_verify)
_DRAFT_CONFIG_KEYS = ("vocab_size", "v_feature_size", "type_vocab_size", "max_position_embeddings")   # policy.check_teacher's

# root(flags [G]) -> (logp [G], id [G]): the model's token 0 (the prefill's copy row) under the flags of step 0
# draft(j, n, token, flags [G], hist) -> id [G]: the draft's greedy token of step n[s] + j, answer token n[s] + j - 1 = token[s]
# verify(n, last, drafts [G, g], flags [G, g + 1], hist) -> (logp [G, g + 1], id [G, g + 1]): the model's token of step n[s] + j
#   after hist[s, :n[s]] (whose last token is last[s]) and drafts[s, :j]
# commit(n, emit [G], live [G]): slot s keeps `emit[s]` of the round's tokens (0 for a slot that was not live)
# n: int64 [G]; hist: int64 [G, W + g + 1], the emitted tokens (read only)
SpecSteps = namedtuple("SpecSteps", "root draft verify commit")
# The sampling loop's: one slot per (dialog, draw), S = G * slots of them in place of G.
# root(flags [S]) -> (logp [S], logq [S], id [S]): the model's plain DRAW of token 0
# draft(j, n, token, flags [S], hist) -> id [S]: the draft's DRAW of step n[s] + j from its filtered distribution Q~
# verify(n, last, drafts [S, g], flags [S, g + 1], hist) -> (logp, logq, id, accept), [S, g + 1] each: row j < g accepts drafts[s, j]
#   with probability min(1, P~ / Q~) (accept = 1, id = the draft) or draws id from the residual; row g is a plain draw of the model
# commit: as above
SpecSampleSteps = namedtuple("SpecSampleSteps", "root draft verify commit")


def pair_keys(i):
    """The new rows that new row i of a slot attends under unimm_attn_verify's rule, in key order."""
    return list(range(0, i // 2 * 2 + 1, 2)) + ([i] if i % 2 else [])


def _rounds(steps, S, limits, W, g, min_answer_len, dev, rejection):
    """The rounds of the module docstring over S slots -> dict(toks [S, W], lp, lq (rejection only), lengths, rounds, drafted,
    accepted, per_round).  rejection: the match mask is the verify step's `accept`, not the equality of draft and model token."""
    WW = W + g + 1                                                          # room for a round's writes past the end: dropped
    toks = torch.zeros((S, WW), dtype=torch.int64, device=dev)
    lp = torch.zeros((S, WW), dtype=F32, device=dev)
    lq = torch.zeros((S, WW), dtype=F32, device=dev) if rejection else None
    ar = torch.arange(S, device=dev)
    jj = torch.arange(g + 1, device=dev)[None]
    root = steps.root(row_flags(torch.zeros_like(limits), limits, min_answer_len))
    toks[:, 0] = root[-1].to(dev, torch.int64)
    lp[:, 0] = root[0].to(dev, F32)
    if rejection:
        lq[:, 0] = root[1].to(dev, F32)
    done = toks[:, 0] == SEP
    n = torch.ones(S, dtype=torch.int64, device=dev)
    drafted = torch.zeros(S, dtype=torch.int64, device=dev)
    accepted = torch.zeros(S, dtype=torch.int64, device=dev)
    record, rounds = [], 0
    while not bool(done.all()):                                             # the round's one device -> host synchronisation
        rounds += 1
        live = ~done
        last = toks[ar, n - 1]
        token, drafts = last, []
        for j in range(g):
            token = steps.draft(j, n, token, row_flags(n + j, limits, min_answer_len), toks).to(dev, torch.int64)
            drafts.append(token)
        drafts = torch.stack(drafts, 1)
        steps_k = n[:, None] + jj
        out = steps.verify(n, last, drafts, row_flags(steps_k, limits[:, None], min_answer_len), toks)
        vals, ids = out[0].to(dev, F32), out[2 if rejection else 1].to(dev, torch.int64)
        if rejection:
            match = torch.cumprod(out[3].to(dev, torch.int64)[:, :g].clamp(0, 1), 1)
        else:
            match = torch.cumprod((drafts == ids[:, :g]).to(torch.int64), 1)
        a_raw = match.sum(1)
        is_sep = (ids == SEP) & (jj <= a_raw[:, None])
        sep_pos = torch.where(is_sep.any(1), is_sep.to(torch.int64).argmax(1), g + 1)
        acc = torch.minimum(a_raw, sep_pos + 1)                              # stops after an accepted [SEP]
        emit = torch.minimum(a_raw + 1, sep_pos + 1)
        acc = torch.where(live, acc, 0)
        emit = torch.where(live, emit, 0)
        keep = jj < emit[:, None]
        toks.scatter_(1, steps_k, torch.where(keep, ids, toks.gather(1, steps_k)))
        lp.scatter_(1, steps_k, torch.where(keep, vals, lp.gather(1, steps_k)))
        if rejection:
            lq.scatter_(1, steps_k, torch.where(keep, out[1].to(dev, F32), lq.gather(1, steps_k)))
        steps.commit(n, emit, live)
        drafted = drafted + torch.where(live, g, 0)
        accepted = accepted + acc
        record.append(torch.where(live, acc, -1))
        n = n + emit
        done = done | (live & (sep_pos <= a_raw))
    return dict(toks=toks[:, :W].contiguous(), lp=lp[:, :W].contiguous(), lq=lq[:, :W].contiguous() if rejection else None,
                lengths=n, rounds=rounds, drafted=drafted, accepted=accepted,
                per_round=torch.stack(record) if record else torch.zeros((0, S), dtype=torch.int64, device=dev))


def speculative_search(steps, G, limits, max_answer_len, draft_len, min_answer_len=1, length_penalty=0.0, device="cpu"):
    """Run the rounds of the module docstring -> GeneratedAnswers shaped like beam_search(beams=1)'s, with `.speculation`."""
    g, W = int(draft_len), max_answer_len + 1
    dev = torch.device(device)
    limits = torch.as_tensor(np.asarray(limits), dtype=torch.int64).to(dev)
    r = _rounds(steps, G, limits, W, g, min_answer_len, dev, False)
    toks, lp, lengths = r["toks"], r["lp"], r["lengths"]
    logp, scores = _greedy_sums(lp, lengths, W, length_penalty, dev)
    spec = Speculation(rounds=r["rounds"], drafted=r["drafted"], accepted=r["accepted"], per_round=r["per_round"])
    return GeneratedAnswers(tokens=toks.view(G, 1, W), lengths=lengths.view(G, 1), scores=scores.view(G, 1), logp=logp.view(G, 1),
                            step_logp=lp.view(G, 1, W), speculation=spec)


def speculative_sample_search(steps, G, samples, limits, max_answer_len, draft_len, min_answer_len=1, length_penalty=0.0,
                              device="cpu", greedy=False):
    """The rounds with the REJECTION rule (SpecSampleSteps) over G * (samples + greedy) slots, slot s = g * slots + j as in
    `generation.sample_search` -> GeneratedAnswers shaped like that function's: the samples in draw order with step_logp and
    step_logq, `.greedy` (shaped and summed like a beams = 1 result) when asked, `.speculation` with [G, samples] counters
    (`.greedy.speculation`: [G])."""
    N, B = int(samples), int(samples) + bool(greedy)
    g, W, S = int(draft_len), max_answer_len + 1, G * B
    dev = torch.device(device)
    limits = torch.as_tensor(np.asarray(limits), dtype=torch.int64).to(dev).repeat_interleave(B)
    r = _rounds(steps, S, limits, W, g, min_answer_len, dev, True)
    toks, lp, lq = (r[k].view(G, B, W) for k in ("toks", "lp", "lq"))
    lengths = r["lengths"].view(G, B)
    drafted, accepted, per = r["drafted"].view(G, B), r["accepted"].view(G, B), r["per_round"].view(-1, G, B)
    spec = lambda j: Speculation(rounds=r["rounds"], drafted=drafted[:, j].contiguous(), accepted=accepted[:, j].contiguous(),  # noqa: E731
                                 per_round=per[:, :, j].contiguous())
    out = sampled_answers(toks, lp, lq, lengths, N, length_penalty,
                          _greedy_sums(lp[:, N].contiguous(), lengths[:, N].contiguous(), W, length_penalty, dev) if greedy else None)
    out.speculation = spec(slice(N))
    if greedy:
        out.greedy.speculation = spec(N)
    return out


def step_streams(streams, k, salts):
    """The stream ids that make ONE launch key its rows by their own steps.  The sampler hashes (key, stream) as
    mix32(key ^ (stream * 0x9E3779B1 + 0x7F4A7C15)), and dropout.make_key(seed, k, site) = site_key(seed, site) ^ step_salt(seed, k);
    the affine map of the stream id is a bijection of the 32-bit words, so a launch keyed by site_key(seed, site) alone with
    stream' = ((stream * A + B) ^ step_salt(seed, k)) - B) * A^-1 draws, for that row, exactly what a launch keyed by
    make_key(seed, k, site) draws for `stream` -- for every site at once.  streams: int32 (any shape); k: int64 steps
    (broadcastable); salts: int64 [>= max k + 1], salts[k] = step_salt(seed, k) -> int32 of the broadcast shape."""
    A, B, M = 0x9E3779B1, 0x7F4A7C15, 0xFFFFFFFF

    def mul32(x, c):                                                         # low 32 bits of x * c without leaving int64
        return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & M

    f = ((mul32(streams.to(torch.int64) & M, A) + B) & M) ^ salts[k.clamp(0, salts.shape[0] - 1)]
    low = mul32((f - B) & M, pow(A, -1, 2 ** 32))
    return torch.where(low >= 2 ** 31, low - 2 ** 32, low).to(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# the refused requests
# ---------------------------------------------------------------------------------------------------------------------------
def check_draft(model, draft, draft_len, beams, samples, no_repeat_ngram_size, repetition_penalty, repeat_scope, accept="match"):
    """The refused uses of `draft` (ValueError, before anything is staged) -> the draft's pre-training model.  accept: "match"
    (greedy: the model keeps the drafts that are its own tokens) or "rejection" (speculative sampling, needs samples >= 1)."""
    from .policy import _pretraining_model
    d = _pretraining_model(draft)
    if not (hasattr(d, "config") and hasattr(d, "_engine") and hasattr(d, "compute_dtype")):
        raise ValueError(f"generate_answers: draft must be a BertForMultiModalPreTraining or a VisualDialogEncoder, got "
                         f"{type(draft).__name__}")
    if d is model or d._engine is model._engine:
        raise ValueError("generate_answers: draft is the model itself (or shares its engine): the two keep separate key/value "
                         "caches; pass a separate model, or policy.frozen_reference(model) to self-draft")
    if int(beams) != 1:
        if accept == "rejection":                # the sampling call's rule, in its words (generation.check_sampling)
            raise ValueError(f"generate_answers: samples > 0 draws independent answers and needs beams = 1, got beams = {beams}")
        raise ValueError(f"generate_answers: draft makes the call speculative GREEDY decoding and needs beams = 1, got beams = {beams}")
    if samples and accept != "rejection":
        raise ValueError(f"generate_answers: draft with samples = {samples}: speculative sampling needs a rejection step on p / q, "
                         "which draft_accept='match' does not take; pass draft_accept='rejection', or drop draft or samples")
    if accept == "rejection" and not samples:
        raise ValueError("generate_answers: draft_accept='rejection' is speculative SAMPLING and needs samples >= 1; for greedy "
                         "decoding use draft_accept='match'")
    if no_repeat_ngram_size or float(np.float32(repetition_penalty)) != 1.0 or repeat_scope != "answer":
        raise ValueError("generate_answers: draft does not take the history rules (no_repeat_ngram_size, repetition_penalty, "
                         "repeat_scope='dialog'): drop draft, or the rules")
    if isinstance(draft_len, bool) or not isinstance(draft_len, (int, np.integer)) or not 1 <= draft_len <= MAX_DRAFT_LEN:
        raise ValueError(f"generate_answers: draft_len must be an integer in [1, {MAX_DRAFT_LEN}] (unimm_attn_verify takes "
                         f"2 * (draft_len + 1) <= 32 rows per dialog), got {draft_len!r}")
    check_model(d, draft=True)
    diff = [k for k in _DRAFT_CONFIG_KEYS if getattr(d.config, k, None) != getattr(model.config, k, None)]
    if diff:
        raise ValueError("generate_answers: draft must read the model's inputs and predict over its vocabulary; its config differs "
                         f"in {', '.join(diff)}")
    if d._device() != model._device():
        raise ValueError(f"generate_answers: draft is on {d._device()}, the model on {model._device()}: move it with .to()")
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# the engines' step functions
# ---------------------------------------------------------------------------------------------------------------------------
def speculate(eng, deng, inp, c_h, limits, draft_len, max_answer_len, min_answer_len, length_penalty, banned_tokens, sampling=None):
    """The engines' step functions of `speculative_search` (sampling None) or of `speculative_sample_search` (sampling: the dict
    `generate_answers` builds, with per-slot `rows`); runs on the model's text stream, the draft's engine entries on the draft's
    (the same stream unless an engine keeps a stream of its own for the text side)."""
    dev = eng.arena.device
    g = int(draft_len)
    banned = torch.tensor(banned_tokens, dtype=torch.int32, device=dev) if banned_tokens else None
    pcap = max(int(limits.max()), 1)
    B = sampling["samples"] + sampling["greedy"] if sampling is not None else 1
    tgt = DecodeSide(eng, inp, c_h, limits, pcap, banned, B, 1)             # every slot an attention group of its own
    drf = deng._on_text_stream(DecodeSide, deng, inp, c_h, limits, pcap + g, banned, B, 1)
    G, S = tgt.G, tgt.S
    V = eng.cfg.vocab_size
    ones = torch.ones(S, dtype=torch.int64, device=dev)
    st = dict(round=0)
    if sampling is not None:
        from . import dropout as DR
        seed, Vpad = sampling["seed"], tgt.pre["logits"].shape[1]
        k_draft, k_accept, k_residual = (DR.site_key(seed, site) for site in (DRAFT_SITE, ACCEPT_SITE, RESIDUAL_SITE))
        salts = torch.tensor([DR.step_salt(seed, k) for k in range(max_answer_len + g + 3)], dtype=torch.int64, device=dev)
        streams = torch.from_numpy(sampling["streams"]).to(dev)
        par = [torch.from_numpy(a).to(dev) for a in sampling["rows"]]                    # per slot: the draft's draws use them too
        par_v = [a.repeat_interleave(g + 1) for a in par]                                # per verified row
        xd = torch.zeros((S, g + 1, Vpad), dtype=F32, device=dev)        # the draft's logits rows of the round (row g: never read)
        dtok = torch.full((S, g + 1), -1, dtype=torch.int32, device=dev)
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)    # noqa: E731
        f32 = lambda n: torch.empty(n, dtype=F32, device=dev)            # noqa: E731
        d_tok, d_lp, d_lq = i32(S), f32(S), f32(S)
        v_acc, v_tok, v_lp, v_lq, v_lse = i32(S * (g + 1)), i32(S * (g + 1)), f32(S * (g + 1)), f32(S * (g + 1)), f32(S * (g + 1))

    def root(flags):
        if sampling is None:
            v, t = tgt.top1(tgt.pre["logits"], G, flags, 1)
            return v.clone(), t.clone()
        logits = tgt.pre["logits"].repeat_interleave(B, 0) if B > 1 else tgt.pre["logits"]
        L.lm_sample_rows(logits, S, V, banned, flags.contiguous(), SEP, par[0], par[1], par[2], k_residual,
                         step_streams(streams, torch.zeros_like(ones), salts), d_tok, d_lp, d_lq)
        return d_lp.clone(), d_lq.clone(), d_tok.clone()

    def draft_step(j, n, token, flags, hist):
        if j == 0:
            st["round"] += 1
        if j == 0 and st["round"] > 1:                                       # plen = n - 2, the pairs of answer rows n-2 and n-1
            drf.plen[drf.cur].copy_((n - 2).clamp_min(0))
            prev = hist.gather(1, (n - 2).clamp_min(0)[:, None])[:, 0]
            tokens, k, P = torch.stack([prev, token], 1), torch.stack([n - 1, n], 1), 2
        else:
            tokens, k, P = token[:, None], (n + j)[:, None], 1
        logits = drf.rows(tokens, k, [P - 1])
        if sampling is None:
            _, t = drf.top1(logits, S, flags, P)
        else:                                                                # a draw from Q~, and the row it was drawn from
            L.lm_sample_rows(logits, S, V, banned, flags.contiguous(), SEP, par[0], par[1], par[2], k_draft,
                             step_streams(streams, n + j, salts), d_tok, d_lp, d_lq)
            xd[:, j].copy_(logits)
            dtok[:, j].copy_(d_tok)
            t = d_tok
        t = t.to(torch.int64).clamp_min(0)
        drf.append(ones * P, P)                                              # (a finished slot's rows are computed and dropped)
        return t

    def draft(j, n, token, flags, hist):
        return deng._on_text_stream(draft_step, j, n, token, flags, hist)

    def verify(n, last, drafts, flags, hist):
        tokens = torch.cat([last[:, None], drafts], 1)
        k = n[:, None] + torch.arange(g + 1, device=dev)[None]
        logits = tgt.rows(tokens, k, list(range(g + 1)))
        if sampling is None:
            v, t = tgt.top1(logits, S * (g + 1), flags, g + 1)
            return v.view(S, g + 1), t.view(S, g + 1)
        L.lm_spec_verify(logits, xd.view(S * (g + 1), Vpad), S * (g + 1), V, dtok.view(-1), banned, flags.reshape(-1).contiguous(), SEP,
                         par_v[0], par_v[1], par_v[2], k_accept, k_residual, step_streams(streams[:, None], k, salts).reshape(-1),
                         v_acc, v_tok, v_lp, v_lq, v_lse)
        return tuple(a.view(S, g + 1) for a in (v_lp, v_lq, v_tok.clamp_min(0), v_acc))

    def commit(n, emit, live):
        tgt.append(emit, g + 1)

    assert V <= tgt.pre["logits"].shape[1]
    if sampling is None:
        return speculative_search(SpecSteps(root, draft, verify, commit), G, limits, max_answer_len, g, min_answer_len,
                                  length_penalty, device=dev)
    return speculative_sample_search(SpecSampleSteps(root, draft, verify, commit), G, sampling["samples"], limits, max_answer_len, g,
                                     min_answer_len, length_penalty, device=dev, greedy=sampling["greedy"])
