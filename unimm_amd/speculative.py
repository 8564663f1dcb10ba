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
`speculate` supplies the engines'.  The Python wrappers of the entry points live here, not in `lib.py`: answer generation is
outside the stream-order check.

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

Slots and groups.  `unimm_attn_verify` takes beams * nr <= 32 query rows per group, so every slot is a group of its own (G' = S,
beams = 1, the dialog's context range, region range and key mask repeated per slot): draft_len <= 15 holds for any samples <= 16,
and no attention kernel changes.  `_Side` keeps S slots over a prefill of G dialogs.

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

import ctypes as C
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

from . import lib as L
from . import params as PM
from .generation import (BF16, F32, MASK, SEP, SEP_BANNED, SEP_FORCED, GeneratedAnswers, Speculation)
from .inputs import DialogMaskSpec

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


def row_flags(k, limits, min_answer_len):
    """int32 flags (any shape) of rows that stand at step k (int64, same shape as limits or broadcastable to it)."""
    return (torch.where(limits <= k, SEP_FORCED, 0) | torch.where(k < min_answer_len, SEP_BANNED, 0)).to(torch.int32)


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


def _greedy_sums(lp, lengths, W, length_penalty, dev):
    """beam_search's arithmetic of one slot per row: logp summed in step order in fp32, scores = logp / length ** penalty."""
    logp = torch.zeros(lp.shape[0], dtype=F32, device=dev)
    for k in range(W):
        logp = torch.where(lengths > k, logp + lp[:, k], logp)
    div = torch.tensor([float((k + 1) ** length_penalty) for k in range(W)], dtype=F32, device=dev)
    return logp, logp / div[lengths - 1]


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
    logp = lp.sum(2)
    scores = logp / lengths.clamp_min(1).to(F32) ** float(length_penalty)
    drafted, accepted, per = r["drafted"].view(G, B), r["accepted"].view(G, B), r["per_round"].view(-1, G, B)
    out = GeneratedAnswers(tokens=toks[:, :N].contiguous(), lengths=lengths[:, :N].contiguous(), scores=scores[:, :N].contiguous(),
                           logp=logp[:, :N].contiguous(), step_logp=lp[:, :N].contiguous(), step_logq=lq[:, :N].contiguous(),
                           speculation=Speculation(rounds=r["rounds"], drafted=drafted[:, :N].contiguous(),
                                                   accepted=accepted[:, :N].contiguous(), per_round=per[:, :, :N].contiguous()))
    if greedy:
        glp, glen = lp[:, N].contiguous(), lengths[:, N].contiguous()
        gsum, gscore = _greedy_sums(glp, glen, W, length_penalty, dev)
        out.greedy = GeneratedAnswers(tokens=toks[:, N:].contiguous(), lengths=glen.view(G, 1), scores=gscore.view(G, 1),
                                      logp=gsum.view(G, 1), step_logp=glp.view(G, 1, W),
                                      speculation=Speculation(rounds=r["rounds"], drafted=drafted[:, N].contiguous(),
                                                              accepted=accepted[:, N].contiguous(), per_round=per[:, :, N].contiguous()))
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
    if d.compute_dtype != "bf16":
        raise ValueError(f"generate_answers: draft must run on the bf16 engine (compute_dtype='bf16'), got {d.compute_dtype!r}")
    if not d.config.with_coattention:
        raise ValueError("generate_answers: draft needs the connection layers (with_coattention)")
    D = d.config.hidden_size // d.config.num_attention_heads
    if D != 64:
        raise ValueError(f"generate_answers: draft's text head size {D} (unimm_attn_decode takes 64)")
    diff = [k for k in _DRAFT_CONFIG_KEYS if getattr(d.config, k, None) != getattr(model.config, k, None)]
    if diff:
        raise ValueError("generate_answers: draft must read the model's inputs and predict over its vocabulary; its config differs "
                         f"in {', '.join(diff)}")
    if d._device() != model._device():
        raise ValueError(f"generate_answers: draft is on {d._device()}, the model on {model._device()}: move it with .to()")
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# the two entry points
# ---------------------------------------------------------------------------------------------------------------------------
def attn_verify(q, k, v, out, ctx_k, ctx_v, ctx_off, ctx_len, priv_k, priv_v, plen, G, beams, nr, H, pcap, scale, D=64):
    """unimm_attn_verify: the arguments of `lib.attn_decode`; nr even, the new rows of a slot are nr / 2 (answer, copy) pairs."""
    L._dev(q, k, v, out, ctx_k, ctx_v, ctx_off, ctx_len, priv_k, priv_v, plen)
    a = L.AttnDecodeArgs()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.ctx_k, a.ctx_v, a.ctx_off, a.ctx_len = ctx_k.data_ptr(), ctx_v.data_ptr(), ctx_off.data_ptr(), ctx_len.data_ptr()
    a.priv_k, a.priv_v, a.plen = L._ptr(priv_k), L._ptr(priv_v), plen.data_ptr()
    a.G, a.beams, a.nr, a.H, a.D, a.pcap = G, beams, nr, H, D, pcap
    a.ldq, a.ldk, a.ldv, a.ldo, a.ldc = q.stride(0), k.stride(0), v.stride(0), out.stride(0), ctx_k.stride(0)
    if ctx_v.stride(0) != ctx_k.stride(0):
        raise L.UnimmHipError("attn_verify: ctx_k and ctx_v need one row stride")
    a.ldp = priv_k.stride(0) if priv_k is not None else 0
    if priv_v is not None and priv_v.stride(0) != a.ldp:
        raise L.UnimmHipError("attn_verify: priv_k and priv_v need one row stride")
    a.scale = scale
    L._call("unimm_attn_verify", C.byref(a))


def kv_cache_append(cache, new_kv, count, plen, plen_out, layers, slots, pcap, width, max_count, new_layer_stride, new_row_mul,
                    new_row_step):
    """unimm_kv_cache_append.  cache: bf16 [layers, slots, pcap, ldp]; new_kv: 2-D bf16 view (row stride = stride(0)) at the first
    K column of layer 0's new rows; new row j of slot s is row s * new_row_mul + j * new_row_step."""
    L._dev(cache, new_kv, count, plen, plen_out)
    a = L.KvAppendArgs()
    a.cache, a.new_kv = cache.data_ptr(), new_kv.data_ptr()
    a.count, a.plen, a.plen_out = count.data_ptr(), plen.data_ptr(), plen_out.data_ptr()
    a.layers, a.slots, a.pcap, a.ldp, a.width, a.max_count = layers, slots, pcap, cache.shape[-1], width, max_count
    a.new_layer_stride, a.ld_new, a.new_row_mul, a.new_row_step = new_layer_stride, new_kv.stride(0), new_row_mul, new_row_step
    L._call("unimm_kv_cache_append", C.byref(a))


def lm_spec_verify(x, xd, rows, V, draft_token, banned, flags, sep, temperature, top_k, top_p, key_accept, key_residual, streams,
                   accept, token, logp, logq, lse, log_ratio=None):
    """unimm_lm_spec_verify: accept the draft's token of every row with probability min(1, P~ / Q~) or draw from the residual.
    x / xd: fp32 logits [rows, >= V] of the model and the draft (2-D views, row stride = stride(0)); draft_token int32 [rows]
    (-1: no draft, a plain draw keyed by key_residual); the rest as `lib.lm_sample_rows`.  accept / token int32 [rows],
    logp / logq / lse (/ log_ratio) fp32 [rows]."""
    L._dev(x, xd, draft_token, banned, flags, temperature, top_k, top_p, streams, accept, token, logp, logq, lse, log_ratio)
    a = L.LmSpecVerifyArgs()
    a.x, a.xd, a.draft_token = L._ptr(x), L._ptr(xd), L._ptr(draft_token)
    a.banned, a.flags, a.stream_ids = L._ptr(banned), L._ptr(flags), L._ptr(streams)
    a.temperature, a.top_k, a.top_p = L._ptr(temperature), L._ptr(top_k), L._ptr(top_p)
    a.accept, a.token = L._ptr(accept), L._ptr(token)
    a.logp, a.logq, a.lse, a.log_ratio = L._ptr(logp), L._ptr(logq), L._ptr(lse), L._ptr(log_ratio)
    a.rows, a.V, a.ldl, a.ldd = rows, V, x.stride(0) if x is not None else 0, xd.stride(0) if xd is not None else 0
    a.nbanned, a.sep = 0 if banned is None else banned.numel(), sep
    a.key_accept, a.key_residual = key_accept & 0xFFFFFFFF, key_residual & 0xFFFFFFFF
    L._call("unimm_lm_spec_verify", C.byref(a))


# ---------------------------------------------------------------------------------------------------------------------------
# the engines' step functions
# ---------------------------------------------------------------------------------------------------------------------------
class _Side:
    """One model's side of a speculative call: the prefill of the G dialogs and its caches, the private cache of every slot
    (B slots per dialog, slot s = g * B + j, all reading dialog g's context), and `rows`: P pairs of new rows per slot through the
    blocks (the decode step of `generation._generate` with 2 P rows per slot).  Text self-attention takes every slot as a group of
    its own (`unimm_attn_verify` with G' = S, beams = 1 and the dialog's context range repeated per slot), so 2 P <= 32 bounds the
    pairs whatever B is; so do the connection layers (the dialog's region range and key mask repeated per slot)."""

    def __init__(self, eng, inp, c_h, limits, pcap, banned, B=1):
        from .scoring import _forward_shared
        self.eng, cfg, dev = eng, eng.cfg, eng.arena.device
        self.cfg, self.dev = cfg, dev
        ids = inp["input_ids"].to(dev, non_blocking=True)
        G, T = ids.shape
        self.G, self.T, self.R = G, T, inp["image_feat"].shape[1]
        self.B, self.S = B, G * B
        S = self.S
        ar = torch.arange(G, device=dev)
        c_d = torch.from_numpy(c_h).to(dev)
        tt = inp.get("token_type_ids")
        tt = tt.to(dev, non_blocking=True).long() if tt is not None else torch.zeros((G, T), dtype=torch.int64, device=dev)
        pp = inp.get("position_ids")
        pp = pp.to(dev, non_blocking=True).long() if pp is not None else torch.arange(T, device=dev).repeat(G, 1)
        pos0, seg0 = pp[ar, c_d - 1] + 1, tt[ar, c_d - 1] ^ 1                         # generation.answer_ids of token 0
        pid, ptt, ppp = ids.long().clone(), tt.clone(), pp.clone()
        lab = torch.full((G, T), -1, dtype=torch.int64, device=dev)
        for j, tok in ((0, SEP), (1, MASK)):
            pid[ar, c_d + j] = tok
            ptt[ar, c_d + j] = seg0
            ppp[ar, c_d + j] = pos0
        lab[ar, c_d + 1] = SEP
        pin = dict(input_ids=pid, image_feat=inp["image_feat"], image_loc=inp["image_loc"], token_type_ids=ptt, position_ids=ppp,
                   masked_lm_labels=lab, attention_mask=DialogMaskSpec(np.ones(G), c_h + 1, np.ones(G)))
        for k in ("image_attention_mask", "image_index"):
            if k in inp:
                pin[k] = inp[k]
        self.cache = {}
        self.pre = _forward_shared(eng, pin, np.arange(G), False, self.cache)
        plan = self.pre["plan"]
        per_slot = (lambda a: a.repeat_interleave(B, 0)) if B > 1 else (lambda a: a)
        self.slot_pos, self.slot_seg = per_slot(pos0), per_slot(seg0)
        self.s_off, self.s_len = (per_slot(torch.from_numpy(a.astype(np.int32)).to(dev)) for a in (plan.s_off, plan.s_len))
        self.sched = PM.encoder_schedule(cfg)
        tkeys = [f"t{i}" for kind, i in self.sched if kind == "t"]
        self.nt, self.lidx = len(tkeys), {key: n for n, key in enumerate(tkeys)}
        self.pcap = pcap
        H = cfg.hidden_size
        self.priv = torch.zeros((self.nt, S, pcap, 2 * H), dtype=BF16, device=dev)
        self.plen = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2)]
        self.cur = 0
        self.limits = per_slot(torch.from_numpy(np.asarray(limits, dtype=np.int64)).to(dev))
        self.banned = banned
        self.k_off = per_slot((ar * self.R).to(torch.int32))
        self.k_len = torch.full((S,), self.R, dtype=torch.int32, device=dev)
        self.vwords = per_slot(self.cache["vwords"])
        self.per_P = {}

    def _buffers(self, P):
        """What depends on the pairs per slot: the per-layer projection stash, the connection layers' query ranges, the scratch
        of the top-1."""
        if P not in self.per_P:
            G, S, B, dev, M = self.G, self.S, self.B, self.dev, self.S * 2 * P
            ar = torch.arange(S, device=dev)
            self.per_P[P] = dict(stash=torch.empty((self.nt, M, 3 * self.cfg.hidden_size), dtype=BF16, device=dev),
                                 q_off=(ar * 2 * P).to(torch.int32), q_len=torch.full((S,), 2 * P, dtype=torch.int32, device=dev),
                                 vals=torch.empty((S * P, 1), dtype=F32, device=dev),
                                 tops=torch.empty((S * P, 1), dtype=torch.int32, device=dev))
        return self.per_P[P]

    def rows(self, tokens, k, decode):
        """tokens int64 [S, P]: the token of answer row k[s, j] - 1; k int64 [S, P]: the step of pair j's copy row.  The slots'
        private rows are [0, plen[cur]).  decode: the pairs whose copy rows are decoded -> fp32 logits [S * len(decode), Vpad]."""
        eng, cfg, dev, G, S = self.eng, self.cfg, self.dev, self.G, self.S
        P = tokens.shape[1]
        M = S * 2 * P
        buf = self._buffers(P)
        H, Hb = cfg.hidden_size, cfg.bi_hidden_size
        heads, nh = cfg.num_attention_heads, cfg.bi_num_attention_heads
        D, Db = H // heads, Hb // nh
        NO = L.NO_DROP
        kc = torch.minimum(k, self.limits[:, None]).clamp_min(0)            # rows past a dialog's limit are dropped: keep their ids inside
        ids32 = torch.stack([tokens, torch.full_like(tokens, MASK)], 2).reshape(M).to(torch.int32)
        pos32 = (self.slot_pos[:, None, None] + torch.stack([(kc - 1).clamp_min(0), kc], 2)).reshape(M).to(torch.int32)
        typ32 = self.slot_seg.repeat_interleave(2 * P).to(torch.int32)
        xt32, xt, _ = eng._embed_text(ids32, pos32, typ32, M, None, NO, False, None)
        plen = self.plen[self.cur]
        for kind, i in self.sched:
            if kind == "t":
                key = f"t{i}"
                qkv_l, so, ff1, ff2 = (eng.lin[key + s] for s in (".qkv", ".so", ".ff1", ".ff2"))
                li = self.lidx[key]
                qkv = eng._linear(xt, qkv_l, out=buf["stash"][li])
                ctxq = self.cache[key]
                ctx = torch.empty((M, H), dtype=BF16, device=dev)
                pv = self.priv[li].view(S * self.pcap, 2 * H)
                attn = L.attn_decode if P == 1 else attn_verify
                attn(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], ctx, ctxq[:, H:2 * H], ctxq[:, 2 * H:], self.s_off, self.s_len,
                     pv[:, :H], pv[:, H:], plen, S, 1, 2 * P, heads, self.pcap, 1.0 / math.sqrt(D))
                xt32, xt = eng._post_attn(ctx, xt32, so, ff1, ff2, key + ".ln1", key + ".ln2", NO, NO, False)[:2]
            elif kind == "c":
                key = f"c{i}"
                lq2, d2, tff1, tff2 = (eng.lin[key + s] for s in (".qkv2", ".d2", ".tff1", ".tff2"))
                qkv1 = self.cache[key]
                qkv2 = eng._linear(xt, lq2)
                ctx_t = torch.empty((M, Hb), dtype=BF16, device=dev)
                vwords = self.vwords
                L.attn_fwd(qkv2[:, :Hb], qkv1[:, Hb:2 * Hb], qkv1[:, 2 * Hb:], ctx_t, None, vwords, S, nh, self.T, self.R, Db,
                           1.0 / math.sqrt(Db), 0, vwords.shape[1], NO, qvar=(buf["q_off"], buf["q_len"]),
                           kvar=(self.k_off, self.k_len))
                xt32, xt = eng._post_attn(ctx_t, xt32, d2, tff1, tff2, key + ".lnb2", key + ".lnt", NO, NO, False)[:2]
        n = S * len(decode)
        sel = (torch.arange(S, device=dev)[:, None] * 2 * P + 2 * torch.as_tensor(decode, device=dev)[None] + 1).reshape(n)
        xs = torch.empty((n, H), dtype=BF16, device=dev)
        L.gather_rows(xt, sel.to(torch.int32), xs, n, H)
        return eng.decode_rows(xs, n)

    def top1(self, logits, rows, flags, P):
        """The greedy token of every row and its log p under the rows' flags (unimm_lm_topk, K = 1) -> (logp [rows], id [rows])."""
        buf = self._buffers(P)
        L.lm_topk(logits, rows, self.cfg.vocab_size, self.banned, flags.reshape(rows).contiguous(), SEP, 1, buf["vals"][:rows],
                  buf["tops"][:rows])
        return buf["vals"][:rows, 0], buf["tops"][:rows, 0]

    def append(self, count, P):
        """Append the first count[s] answer rows the last `rows` call with P pairs pushed to the private cache of slot s."""
        cur, H = self.cur, self.cfg.hidden_size
        stash = self._buffers(P)["stash"]
        kv_cache_append(self.priv, stash[0][:, H:], count.to(torch.int32), self.plen[cur], self.plen[1 - cur], self.nt, self.S,
                        self.pcap, 2 * H, P, stash.shape[1] * 3 * H, 2 * P, 2)
        self.cur = 1 - cur


def speculate(eng, deng, inp, c_h, limits, draft_len, max_answer_len, min_answer_len, length_penalty, banned_tokens, sampling=None):
    """The engines' step functions of `speculative_search` (sampling None) or of `speculative_sample_search` (sampling: the dict
    `generate_answers` builds, with per-slot `rows`); runs on the model's text stream, the draft's engine entries on the draft's
    (the same stream unless an engine keeps a stream of its own for the text side)."""
    dev = eng.arena.device
    g = int(draft_len)
    banned = torch.tensor(banned_tokens, dtype=torch.int32, device=dev) if banned_tokens else None
    pcap = max(int(limits.max()), 1)
    B = sampling["samples"] + sampling["greedy"] if sampling is not None else 1
    tgt = _Side(eng, inp, c_h, limits, pcap, banned, B)
    drf = deng._on_text_stream(_Side, deng, inp, c_h, limits, pcap + g, banned, B)
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
        lm_spec_verify(logits, xd.view(S * (g + 1), Vpad), S * (g + 1), V, dtok.view(-1), banned, flags.reshape(-1).contiguous(), SEP,
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
