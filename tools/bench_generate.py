"""Answer generation throughput at the full config (seeded weights): prefill, decode step, answers/s and tokens/s for
(G, beams) in {(1, 1), (1, 5), (80, 1), (80, 4)}, every answer exactly 20 tokens + [SEP] (min_answer_len = max_answer_len = 20),
against the recompute lower bound: sequence_log_likelihood of the same G * beams sequences at answer lengths 1 .. 20 summed
(a generator that re-runs the encoder per token pays at least that) -- with shared_context=<dialog> where that path applies
(answers of <= 14 tokens: it takes <= 32 private rows per sequence), the per-sequence path for the longer ones.

    python tools/bench_generate.py [--reps 3] [--shapes 1,1 80,4] [--profile] [--samples N]
                                   [--no-repeat-ngram N] [--repetition-penalty R] [--repeat-scope answer|dialog]
                                   [--draft-layers t,v,c --draft-len g [g ...]]
                                   [--ensemble K [--ensemble-mode prob|logit]]

--samples N adds, for G = 80 dialogs: ms/step of sampling N answers per dialog (temperature 0.8, top_k 50, top_p 0.9) against a
beam run with the same number of hypothesis slots (beams = N) in the same process, the time of one unimm_lm_sample launch against
one unimm_lm_topk launch on the same [80 N, 30522] logits, and the two ways of appending a step's K | V rows to the private caches
(tensor indexing in place, which the sampler uses, against unimm_kv_cache_update under an identity parent).

--no-repeat-ngram / --repetition-penalty (either one on) add, at G = 80 and 4 slots per dialog (or --samples): one
unimm_lm_topk_hist launch against one unimm_lm_topk launch and one unimm_lm_sample_hist launch against one unimm_lm_sample_rows
launch on the same [80 slots, 30522] logits (10 answer tokens of history per row, and with --repeat-scope dialog the dialogs'
contexts), and the whole decode loop (20 tokens, beams and samples) with and without the rules -- each as alternating pairs in
one process: the median of the per-pair ratios, and the spread (max / min) of the plain form over the pairs.

--draft-layers t,v,c (text, image and connection layers of a randomly initialised draft) with --draft-len g ... adds, at G = 80:
the time of one plain decode step (two rows per dialog), of one verify pass of the model at each g (2 (g + 1) rows per dialog
through unimm_attn_verify, the head and the top-1 on g + 1 rows), of one decode step of the draft, the break-even acceptance that
follows from the three -- a round costs g draft steps + one verify pass and yields (accepted drafts + 1) tokens, a plain step yields
one -- and the end-to-end time of a speculative call with a frozen copy of the model as the draft against the plain call.  The
copy's acceptance is near 1: that measures the machinery, not a speed-up (no trained student exists).

--samples N together with --draft-layers adds, at G = 80 (speculative SAMPLING, draft_accept="rejection"): one
unimm_lm_spec_verify launch against one unimm_lm_sample_rows launch on the same 80 N (g + 1) rows of [., 30522] logits (the drafts
drawn from the draft rows, xd = x + noise; the byte count beside it: one read of the model row, two of the draft row), and a
rejection-sampled call with a frozen copy as the draft against the plain sampling call (temperature 0.8, top_k 50, top_p 0.9).

--ensemble K (members, 2 .. 5; --ensemble-mode prob or logit) adds, at G = 80: one unimm_lm_mix launch on K blocks of [640, 30522]
logits (row stride 30528) beside one unimm_lm_topk launch on one of them -- microseconds, the bytes the launch moves (every member
row once in logit mode, twice in prob mode, the mixed row written once) and TB/s -- and the call with K - 1 frozen copies of the
model as partners beside the plain call, at beams = 1 and at 8 samples per dialog (temperature 0.8, top_k 50, top_p 0.9).  The
expectation to read the ratios against is K decode steps plus the mix.  The copies measure the machinery: no trained ensemble
exists, and no answer quality is measured.

--profile adds the kernel mix of one call at (80, 4) from a `rocprofv3 --kernel-trace --stats` run of this tool in a child
process (per decode step = the call's launches / 20; the prefill's own kernels run once and are listed with it)."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG_PATH = os.path.join(ROOT, "unimm_amd", "config", "bert_base_6layer_6conect.json")
ANS = 20
T, R, F = 256, 37, 2048


def build_model():
    from oracle import vilbert_ref as RF
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    model = BertForMultiModalPreTraining(BertConfig.from_json_file(CFG_PATH))
    model.load_state_dict(RF.init_state_dict(RF.make_config(CFG_PATH), seed=5), strict=True)
    return model.cuda().eval()


def dialogs(G, seed):
    """G contexts of 60 .. 180 tokens ([CLS] utterances [SEP] ..., segments toggling), random regions, on the device."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((G, T), dtype=np.int64)
    tt = np.zeros((G, T), dtype=np.int64)
    c = np.zeros(G, dtype=np.int64)
    for g in range(G):
        target, toks, segs, s = int(rng.integers(60, 181)), [101], [0], 0
        while len(toks) < target:
            u = rng.integers(1000, 30522, int(rng.integers(3, 12))).tolist() + [102]
            toks += u
            segs += [s] * len(u)
            s ^= 1
        ids[g, :len(toks)], tt[g, :len(toks)], c[g] = toks, segs, len(toks)
    pp = np.tile(np.arange(T), (G, 1))
    d = dict(input_ids=ids, token_type_ids=tt, position_ids=pp)
    d = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    d["image_feat"] = torch.from_numpy(rng.standard_normal((G, R, F)).astype(np.float32)).cuda()
    d["image_loc"] = torch.from_numpy(rng.random((G, R, 5)).astype(np.float32)).cuda()
    d["image_attention_mask"] = torch.ones((G, R), dtype=torch.int64, device="cuda")
    return d, c


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def generate(model, d, c, beams, n, **kw):
    return model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, d["token_type_ids"], d["position_ids"],
                                  d["image_attention_mask"], beams=beams, max_answer_len=n, min_answer_len=n, **kw)


def launch_us(fn, n=50):
    """Microseconds per launch: n launches between two events, after a warm-up."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def measure_sampling(model, G, N, reps):
    """Sampling N answers per dialog against beams = N (the same 2 G N decode rows), and the selection kernels alone."""
    from unimm_amd import lib as L
    d, c = dialogs(G, seed=G * 10 + N)
    skw = dict(samples=N, temperature=0.8, top_k=50, top_p=0.9, seed=1)
    row = dict(G=G, slots=N)
    for name, beams, kw in (("beam", N, {}), ("sample", 1, skw)):
        prefill = timed(lambda: generate(model, d, c, beams, 0, **kw), reps)
        full = timed(lambda: generate(model, d, c, beams, ANS, **kw), reps)
        assert bool((generate(model, d, c, beams, ANS, **kw).lengths == ANS + 1).all())
        row[name + "_prefill_ms"], row[name + "_call_ms"] = round(prefill, 3), round(full, 3)
        row[name + "_ms_per_step"] = round((full - prefill) / ANS, 3)
    S, V = G * N, 30522
    logits = torch.randn((S, V), generator=torch.Generator().manual_seed(0)).cuda() * 3
    banned = torch.tensor([0, 101, 103], dtype=torch.int32, device="cuda")
    flags = torch.zeros(S, dtype=torch.int32, device="cuda")
    streams = torch.arange(S, dtype=torch.int32, device="cuda")
    vals = torch.empty((S, N), dtype=torch.float32, device="cuda")
    ids = torch.empty((S, N), dtype=torch.int32, device="cuda")
    tok = torch.empty(S, dtype=torch.int32, device="cuda")
    lp, lq = torch.empty(S, device="cuda"), torch.empty(S, device="cuda")
    row["lm_topk_us"] = round(launch_us(lambda: L.lm_topk(logits, S, V, banned, flags, 102, N, vals, ids)), 1)
    for name, (t, k, p) in (("lm_sample_us", (0.8, 50, 0.9)), ("lm_sample_plain_us", (1.0, 0, 1.0)), ("lm_sample_top_k_us", (1.0, 50, 1.0)),
                            ("lm_sample_top_p_us", (1.0, 0, 0.9))):
        row[name] = round(launch_us(lambda: L.lm_sample(logits, S, V, banned, flags, 102, t, k, p, 12345, streams, tok, lp, lq)), 1)
    # appending one K | V row per slot and text layer: in place against the copying kernel under an identity parent
    nt, H, pcap = 12, 768, ANS
    priv = [torch.zeros((nt, S, pcap, 2 * H), dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    plen = [torch.full((S,), pcap // 2, dtype=torch.int32, device="cuda") for _ in range(2)]
    stash = torch.randn((nt, 2 * S, 3 * H), device="cuda").to(torch.bfloat16)
    ident = torch.arange(S, dtype=torch.int32, device="cuda")

    def in_place():
        priv[0][:, :, pcap // 2] = stash[:, 0::2, H:]
        plen[0].add_(0)

    row["append_in_place_us"] = round(launch_us(in_place), 1)
    row["append_kv_cache_update_us"] = round(launch_us(lambda: L.kv_cache_update(priv[0], priv[1], stash[0][:, H:], ident, plen[0], plen[1],
                                                                                nt, S, pcap, 2 * H, 2 * S * 3 * H, 2)), 1)
    return row


def paired(plain, ruled, pairs):
    """Alternating pairs plain / ruled -> (median plain, median of the per-pair ratios ruled / plain, max / min of plain)."""
    a, b = [], []
    for _ in range(pairs):
        a.append(plain())
        b.append(ruled())
    a, b = np.asarray(a), np.asarray(b)
    return float(np.median(a)), float(np.median(b / a)), float(a.max() / a.min())


def measure_constraints(model, G, N, reps, ngram, penalty, scope):
    """The cost of the history rules: one _hist launch against the plain launch on the same logits, and the decode loop."""
    from unimm_amd import generation as GN
    from unimm_amd import lib as L
    d, c = dialogs(G, seed=G * 10 + N)
    S, V, HLEN, PAIRS = G * N, 30522, 10, 7
    gen = torch.Generator().manual_seed(0)
    logits = torch.randn((S, V), generator=gen).cuda() * 3
    banned = torch.tensor([0, 101, 103], dtype=torch.int32, device="cuda")
    flags = torch.zeros(S, dtype=torch.int32, device="cuda")
    streams = torch.arange(S, dtype=torch.int32, device="cuda")
    vals = torch.empty((S, N), dtype=torch.float32, device="cuda")
    ids = torch.empty((S, N), dtype=torch.int32, device="cuda")
    tok = torch.empty(S, dtype=torch.int32, device="cuda")
    lp, lq = torch.empty(S, device="cuda"), torch.empty(S, device="cuda")
    t, k, p = (torch.full((S,), v, dtype=dt, device="cuda") for v, dt in ((0.8, torch.float32), (50, torch.int32), (0.9, torch.float32)))
    hist = torch.randint(1000, 1040, (S, ANS), generator=gen, dtype=torch.int32).cuda()      # 40 ids: windows do match
    hlen = torch.full((S,), HLEN, dtype=torch.int32, device="cuda")
    ctx, ctx_len = GN.context_table(d["input_ids"], c) if scope == "dialog" else (None, None)
    ctx_idx = torch.arange(S, dtype=torch.int32, device="cuda") // N if ctx is not None else None
    kpen = penalty if N == 1 else 1.0                                          # a penalised top-K is a beams = 1 launch
    hs = L.lm_history(hist, hlen, ngram, penalty, 102, ctx, ctx_len, ctx_idx)
    hk = L.lm_history(hist, hlen, ngram, kpen, 102, ctx, ctx_len, ctx_idx)
    row = dict(G=G, slots=N, ngram=ngram, penalty=penalty, scope=scope)
    row["lm_topk_us"], row["lm_topk_hist_ratio"], row["lm_topk_spread"] = paired(
        lambda: launch_us(lambda: L.lm_topk(logits, S, V, banned, flags, 102, N, vals, ids)),
        lambda: launch_us(lambda: L.lm_topk_hist(logits, S, V, banned, flags, 102, N, hk, vals, ids)), PAIRS)
    row["lm_sample_rows_us"], row["lm_sample_hist_ratio"], row["lm_sample_rows_spread"] = paired(
        lambda: launch_us(lambda: L.lm_sample_rows(logits, S, V, banned, flags, 102, t, k, p, 12345, streams, tok, lp, lq)),
        lambda: launch_us(lambda: L.lm_sample_hist(logits, S, V, banned, flags, 102, t, k, p, 12345, streams, hs, tok, lp, lq)), PAIRS)
    rules = dict(no_repeat_ngram_size=ngram, repeat_scope=scope)
    for name, beams, kw, pen in (("beam", N, {}, kpen), ("sample", 1, dict(samples=N, temperature=0.8, top_k=50, top_p=0.9, seed=1), penalty)):
        def call(**more):
            t0 = time.perf_counter()
            res = generate(model, d, c, beams, ANS, **kw, **more)
            torch.cuda.synchronize()
            assert bool((res.lengths == ANS + 1).all())
            return (time.perf_counter() - t0) * 1e3
        call(), call(repetition_penalty=pen, **rules)                          # warm-up of both
        row[name + "_call_ms"], row[name + "_ruled_ratio"], row[name + "_call_spread"] = paired(
            call, lambda: call(repetition_penalty=pen, **rules), max(reps, 3))
    return {k: round(v, 4) if isinstance(v, float) else v for k, v in row.items()}


def measure_speculative(model, G, layers, gammas, reps):
    """One plain decode step, one verify pass per draft_len, one step of a random draft of `layers` = (text, image, connection)
    layers, the break-even acceptance, and a speculative call with a frozen copy as the draft."""
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    from unimm_amd import generation as GN
    from unimm_amd.decoding import DecodeSide
    from unimm_amd.policy import frozen_reference
    nt_, nv_, nc_ = layers
    cfgd = json.load(open(CFG_PATH))
    cfgd.update(num_hidden_layers=nt_, v_num_hidden_layers=nv_, t_biattention_id=list(range(nt_ - nc_, nt_)),
                v_biattention_id=list(range(nv_ - nc_, nv_)))
    torch.manual_seed(7)
    small = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd)).cuda().eval()
    d, c = dialogs(G, seed=G * 10 + 1)
    limits = GN.answer_limits(c, T, ANS)
    banned = torch.tensor([0, 101, 103], dtype=torch.int32, device="cuda")
    inp = dict(input_ids=d["input_ids"], image_feat=d["image_feat"], image_loc=d["image_loc"], token_type_ids=d["token_type_ids"],
               position_ids=d["position_ids"], image_attention_mask=d["image_attention_mask"])
    gen = torch.Generator().manual_seed(0)

    def side_of(m, pcap):
        eng = m._engine
        eng.ensure(m._device())
        with torch.no_grad():
            side = eng._on_text_stream(DecodeSide, eng, dict(inp), c, limits, pcap, banned, 1, 1)   # the beams = 1 call's side
        side.plen[side.cur].fill_(ANS // 2)                                  # the middle of an answer: 10 private rows
        return side

    def pass_ms(side, P):
        tokens = torch.randint(1000, 30522, (G, P), generator=gen).cuda()
        k = (ANS // 2 + 1 + torch.arange(P, device="cuda"))[None].expand(G, P).contiguous()
        flags = torch.zeros(G * P, dtype=torch.int32, device="cuda")

        def run():
            with torch.no_grad():
                side.eng._on_text_stream(lambda: side.top1(side.rows(tokens, k, list(range(P))), G * P, flags, P))
        return launch_us(run, n=max(10, 10 * reps)) / 1e3

    tgt, drf = side_of(model, ANS), side_of(small, ANS + max(gammas))
    plain_ms, draft_ms = pass_ms(tgt, 1), pass_ms(drf, 1)
    copy = frozen_reference(model)
    call_plain = timed(lambda: generate(model, d, c, 1, ANS), reps)
    row = dict(G=G, draft_layers=list(layers), plain_step_ms=round(plain_ms, 4), draft_step_ms=round(draft_ms, 4),
               plain_call_ms=round(call_plain, 3), per_draft_len=[])
    for g in gammas:
        verify_ms = pass_ms(tgt, g + 1)
        need = (g * draft_ms + verify_ms) / plain_ms - 1.0                   # accepted drafts per round at which a round pays
        lo, hi = 0.0, 1.0                                                    # ... and the per-token acceptance with that mean
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if sum(mid ** j for j in range(1, g + 1)) < need else (lo, mid)
        res = generate(model, d, c, 1, ANS, draft=copy, draft_len=g)
        assert bool((res.lengths == ANS + 1).all())
        sp = res.speculation
        call = timed(lambda: generate(model, d, c, 1, ANS, draft=copy, draft_len=g), reps)
        row["per_draft_len"].append(dict(
            draft_len=g, verify_ms=round(verify_ms, 4), verify_over_plain=round(verify_ms / plain_ms, 3),
            break_even_accepted_per_round=round(need, 3), break_even_token_acceptance=(round(hi, 3) if need < g else None),
            copy_call_ms=round(call, 3), copy_call_over_plain=round(call / call_plain, 3), copy_rounds=sp.rounds,
            copy_acceptance=round(float(sp.accepted.sum()) / max(float(sp.drafted.sum()), 1.0), 3)))
    return row


def measure_spec_sampling(model, G, N, gammas, reps):
    """The rejection step alone (one launch against the sampler's on the same rows) and a rejection-sampled call with a frozen copy
    as the draft against the plain sampling call."""
    from unimm_amd import lib as L
    from unimm_amd.policy import frozen_reference
    d, c = dialogs(G, seed=G * 10 + N)
    V, PAIRS = 30522, 5
    skw = dict(samples=N, temperature=0.8, top_k=50, top_p=0.9, seed=1)
    copy = frozen_reference(model)
    call_plain = timed(lambda: generate(model, d, c, 1, ANS, **skw), reps)
    row = dict(G=G, samples=N, plain_call_ms=round(call_plain, 3), per_draft_len=[])
    banned = torch.tensor([0, 101, 103], dtype=torch.int32, device="cuda")
    for g in gammas:
        rows = G * N * (g + 1)
        gen = torch.Generator().manual_seed(g)
        x = torch.randn((rows, V), generator=gen).cuda() * 3
        xd = x + torch.randn((rows, V), generator=gen).cuda() * 0.5
        flags = torch.zeros(rows, dtype=torch.int32, device="cuda")
        streams = torch.arange(rows, dtype=torch.int32, device="cuda")
        t, k, p = (torch.full((rows,), v, dtype=dt, device="cuda") for v, dt in ((0.8, torch.float32), (50, torch.int32), (0.9, torch.float32)))
        dtok, acc, tok = (torch.empty(rows, dtype=torch.int32, device="cuda") for _ in range(3))
        lp, lq, lse = (torch.empty(rows, device="cuda") for _ in range(3))
        L.lm_sample_rows(xd, rows, V, banned, flags, 102, t, k, p, 777, streams, dtok, lp, lq)
        sample_us, ratio, spread = paired(
            lambda: launch_us(lambda: L.lm_sample_rows(x, rows, V, banned, flags, 102, t, k, p, 12345, streams, tok, lp, lq), n=20),
            lambda: launch_us(lambda: L.lm_spec_verify(x, xd, rows, V, dtok, banned, flags, 102, t, k, p, 999, 12345, streams, acc, tok,
                                                       lp, lq, lse), n=20), PAIRS)
        accepted = float(acc.float().mean())
        del x, xd
        res = generate(model, d, c, 1, ANS, draft=copy, draft_len=g, draft_accept="rejection", **skw)
        assert bool((res.lengths == ANS + 1).all())
        sp = res.speculation
        call = timed(lambda: generate(model, d, c, 1, ANS, draft=copy, draft_len=g, draft_accept="rejection", **skw), reps)
        row["per_draft_len"].append(dict(
            draft_len=g, rows=rows, lm_sample_rows_us=round(sample_us, 1), spec_verify_over_sample_rows=round(ratio, 3),
            sample_rows_spread=round(spread, 3), launch_acceptance=round(accepted, 3),
            mib_read=round(rows * V * 4 * 3 / 2 ** 20, 1), gb_per_s=round(rows * V * 4 * 3 / (sample_us * ratio * 1e-6) / 1e9, 1),
            copy_call_ms=round(call, 3), copy_call_over_plain=round(call / call_plain, 3), copy_rounds=sp.rounds,
            copy_acceptance=round(float(sp.accepted.sum()) / max(float(sp.drafted.sum()), 1.0), 3)))
    return row


def measure_ensemble(model, G, K, mode, reps):
    """One unimm_lm_mix launch beside one unimm_lm_topk launch on the same rows, and the call with K - 1 frozen copies as partners
    beside the plain call: greedy and 8 samples per dialog."""
    from unimm_amd import lib as L
    from unimm_amd import mix as MX
    from unimm_amd.policy import frozen_reference
    N, V, LD, PAIRS = 8, 30522, 30528, 5
    S = G * N
    gen = torch.Generator().manual_seed(0)
    blocks = [(torch.randn((S, LD), generator=gen) * 3).cuda() for _ in range(K)]
    out = torch.empty((S, LD), device="cuda")
    banned = torch.tensor([0, 101, 103], dtype=torch.int32, device="cuda")
    flags = torch.zeros(S, dtype=torch.int32, device="cuda")
    vals = torch.empty((S, 1), dtype=torch.float32, device="cuda")
    ids = torch.empty((S, 1), dtype=torch.int32, device="cuda")
    weights = [1.0 / K] * K
    row = dict(G=G, members=K, mode=mode, rows=S)
    topk_us, ratio, spread = paired(
        lambda: launch_us(lambda: L.lm_topk(blocks[0], S, V, banned, flags, 102, 1, vals, ids), n=20),
        lambda: launch_us(lambda: MX.lm_mix(blocks, weights, mode, V, banned, flags, 102, float("-inf"), out), n=20), PAIRS)
    nbytes = S * V * 4 * (K * (2 if mode == "prob" else 1) + 1)
    mix_us = topk_us * ratio
    row.update(lm_topk_us=round(topk_us, 1), lm_mix_us=round(mix_us, 1), lm_mix_over_topk=round(ratio, 3), lm_topk_spread=round(spread, 3),
               lm_mix_mib=round(nbytes / 2 ** 20, 1), lm_mix_tb_per_s=round(nbytes / (mix_us * 1e-6) / 1e12, 3))
    cut_us = launch_us(lambda: MX.lm_mix(blocks, weights, mode, V, banned, flags, 102, float(np.log(0.1)), out), n=20)
    row["lm_mix_cut_us"] = round(cut_us, 1)
    del blocks, out
    d, c = dialogs(G, seed=G * 10 + 1)
    partners = [frozen_reference(model) for _ in range(K - 1)]
    ekw = dict(ensemble=partners, ensemble_mode=mode)
    for name, kw in (("greedy", {}), ("sample", dict(samples=N, temperature=0.8, top_k=50, top_p=0.9, seed=1))):
        def call(**more):
            t0 = time.perf_counter()
            res = generate(model, d, c, 1, ANS, **kw, **more)
            torch.cuda.synchronize()
            assert bool((res.lengths == ANS + 1).all())
            return (time.perf_counter() - t0) * 1e3
        call(), call(**ekw)                                                  # warm-up of both
        row[name + "_call_ms"], row[name + "_ensemble_ratio"], row[name + "_call_spread"] = paired(call, lambda: call(**ekw), max(reps, 3))
    return {k: round(v, 4) if isinstance(v, float) else v for k, v in row.items()}


def recompute_bound(model, d, c, G, beams, reps):
    """Summed ms of scoring G * beams sequences with answers of 1 .. ANS tokens (shared context up to 14 answer tokens)."""
    from unimm_amd.inputs import DialogMaskSpec
    B = G * beams
    gi = np.repeat(np.arange(G), beams)
    rng = np.random.default_rng(1)
    total = 0.0
    for n in range(1, ANS + 1):
        ids = d["input_ids"][gi].clone()
        tt = d["token_type_ids"][gi].clone()
        pp = d["position_ids"][gi].clone()
        lab = torch.full((B, T), -1, dtype=torch.int64, device="cuda")
        ans = torch.from_numpy(rng.integers(1000, 30522, (B, n))).cuda()
        for b in range(B):
            cb = int(c[gi[b]])
            L = cb + n + 1
            seq = torch.cat([ans[b], torch.tensor([102], device="cuda")])
            ids[b, cb:L] = seq
            ids[b, L:L + n + 1] = 103
            lab[b, L:L + n + 1] = seq
            tt[b, cb:L + n + 1] = tt[b, cb - 1] ^ 1
            pp[b, cb:L] = torch.arange(cb, L, device="cuda")
            pp[b, L:L + n + 1] = torch.arange(cb, L, device="cuda")
        spec = DialogMaskSpec(np.ones(B), c[gi] + n + 1, np.full(B, n + 1))
        grp = torch.from_numpy(gi).cuda() if 2 * (n + 1) + 1 <= 32 else None
        total += timed(lambda: model.sequence_log_likelihood(ids, d["image_feat"][gi], d["image_loc"][gi], lab, shared_context=grp,
                                                             token_type_ids=tt, position_ids=pp, attention_mask=spec,
                                                             image_attention_mask=d["image_attention_mask"][gi]), reps)
    return total


def measure(model, G, beams, reps, recompute=True):
    d, c = dialogs(G, seed=G * 10 + beams)
    prefill = timed(lambda: generate(model, d, c, beams, 0), reps)
    full = timed(lambda: generate(model, d, c, beams, ANS), reps)
    res = generate(model, d, c, beams, ANS)
    assert bool((res.lengths == ANS + 1).all())
    step = (full - prefill) / ANS
    row = dict(G=G, beams=beams, prefill_ms=round(prefill, 3), decode_step_ms=round(step, 3), call_ms=round(full, 3),
               answers_per_s=round(G * beams / full * 1e3, 1), tokens_per_s=round(G * beams * (ANS + 1) / full * 1e3, 1))
    if recompute:
        rb = recompute_bound(model, d, c, G, beams, reps)
        row.update(recompute_bound_ms=round(rb, 3), speedup_vs_recompute=round(rb / full, 2))
    return row


def profile():
    """Kernel mix of one (80, 4) call from rocprofv3 --kernel-trace --stats on a child process."""
    out = tempfile.mkdtemp(prefix="bench_generate_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "gen", "--", sys.executable, os.path.abspath(__file__),
           "--shapes", "80,4", "--reps", "1", "--no-recompute", "--quiet"]
    subprocess.run(cmd, check=True, timeout=900)
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        raise RuntimeError(f"no kernel_stats.csv under {out}")
    rows = list(csv.DictReader(open(stats[0])))
    # the profiled process ran the (80, 4) call 1 (warm-up) + 1 (timed) times at 0 and at ANS tokens, + 1 checked call at ANS
    calls_ans = 3
    mix = []
    for r in rows:
        name = r.get("Name") or r.get("KernelName")
        n = int(r.get("Calls", 0))
        ms = float(r.get("TotalDurationNs", 0)) / 1e6
        mix.append(dict(kernel=name[:90], calls_per_step=round(n / (calls_ans * ANS), 2), ms_per_step=round(ms / (calls_ans * ANS), 4)))
    mix.sort(key=lambda m: -m["ms_per_step"])
    return mix[:20]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=["1,1", "1,5", "80,1", "80,4"])
    ap.add_argument("--no-recompute", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--samples", type=int, default=0, help="add the sampling comparison at G = 80 with this many samples per dialog")
    ap.add_argument("--no-repeat-ngram", type=int, default=0, help="add the cost of the history rules at G = 80 with this n-gram size")
    ap.add_argument("--repetition-penalty", type=float, default=1.0, help="... and / or with this repetition penalty")
    ap.add_argument("--repeat-scope", choices=("answer", "dialog"), default="answer")
    ap.add_argument("--draft-layers", default=None, help="t,v,c: add the speculative-decoding measurements at G = 80 with a random draft "
                    "of that many text, image and connection layers")
    ap.add_argument("--draft-len", type=int, nargs="+", default=[4], help="... at these draft lengths")
    ap.add_argument("--ensemble", type=int, default=0, help="add the ensemble measurements at G = 80 with this many members (2 .. 5)")
    ap.add_argument("--ensemble-mode", choices=("prob", "logit"), default="prob")
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = build_model()
    rows = [measure(model, *map(int, s.split(",")), a.reps, recompute=not a.no_recompute) for s in a.shapes]
    if a.quiet:
        return
    print(f"{'G':>3} {'beams':>5} {'prefill ms':>10} {'ms/step':>8} {'call ms':>8} {'answers/s':>10} {'tokens/s':>9} {'recompute ms':>12} {'x':>6}")
    for r in rows:
        print(f"{r['G']:>3} {r['beams']:>5} {r['prefill_ms']:>10.2f} {r['decode_step_ms']:>8.2f} {r['call_ms']:>8.1f} "
              f"{r['answers_per_s']:>10.1f} {r['tokens_per_s']:>9.1f} {r.get('recompute_bound_ms', float('nan')):>12.1f} "
              f"{r.get('speedup_vs_recompute', float('nan')):>6.2f}")
    result = dict(rows=rows)
    if a.samples:
        result["sampling"] = r = measure_sampling(model, 80, a.samples, a.reps)
        print(f"G = {r['G']}, {r['slots']} slots per dialog: ms/step sampling {r['sample_ms_per_step']:.2f} against beams {r['beam_ms_per_step']:.2f}; "
              f"one launch on [{r['G'] * r['slots']}, 30522]: unimm_lm_sample {r['lm_sample_us']:.1f} us (no filter {r['lm_sample_plain_us']:.1f}, "
              f"top-k only {r['lm_sample_top_k_us']:.1f}, nucleus only {r['lm_sample_top_p_us']:.1f}) against unimm_lm_topk {r['lm_topk_us']:.1f} us; "
              f"cache append in place {r['append_in_place_us']:.1f} us against unimm_kv_cache_update {r['append_kv_cache_update_us']:.1f} us")
    if a.no_repeat_ngram or a.repetition_penalty != 1.0:
        result["constraints"] = r = measure_constraints(model, 80, a.samples or 4, a.reps, a.no_repeat_ngram, a.repetition_penalty,
                                                        a.repeat_scope)
        print(f"history rules (n-gram {r['ngram']}, penalty {r['penalty']}, scope {r['scope']}) at G = {r['G']}, {r['slots']} slots per "
              f"dialog, median ratio over alternating pairs (spread of the plain form, max / min): "
              f"unimm_lm_topk_hist / unimm_lm_topk {r['lm_topk_hist_ratio']:.3f} ({r['lm_topk_us']:.1f} us, spread {r['lm_topk_spread']:.3f}); "
              f"unimm_lm_sample_hist / unimm_lm_sample_rows {r['lm_sample_hist_ratio']:.3f} ({r['lm_sample_rows_us']:.1f} us, spread "
              f"{r['lm_sample_rows_spread']:.3f}); decode loop with / without the rules: beams {r['beam_ruled_ratio']:.3f} "
              f"({r['beam_call_ms']:.1f} ms, spread {r['beam_call_spread']:.3f}), samples {r['sample_ruled_ratio']:.3f} "
              f"({r['sample_call_ms']:.1f} ms, spread {r['sample_call_spread']:.3f})")
    if a.draft_layers:
        result["speculative"] = r = measure_speculative(model, 80, tuple(int(x) for x in a.draft_layers.split(",")), a.draft_len, a.reps)
        print(f"speculative decoding at G = {r['G']}: plain decode step {r['plain_step_ms']:.3f} ms, step of a random "
              f"{'+'.join(map(str, r['draft_layers']))}-layer draft {r['draft_step_ms']:.3f} ms, plain call {r['plain_call_ms']:.1f} ms")
        for q in r["per_draft_len"]:
            print(f"  draft_len {q['draft_len']:>2}: verify pass {q['verify_ms']:.3f} ms = {q['verify_over_plain']:.2f} x a plain step; a round "
                  f"pays above {q['break_even_accepted_per_round']:.2f} accepted drafts (per-token acceptance "
                  f"{q['break_even_token_acceptance']}); frozen copy as draft: {q['copy_call_ms']:.1f} ms = {q['copy_call_over_plain']:.2f} x "
                  f"the plain call, {q['copy_rounds']} rounds, acceptance {q['copy_acceptance']:.3f}")
    if a.draft_layers and a.samples:
        result["speculative_sampling"] = r = measure_spec_sampling(model, 80, a.samples, a.draft_len, a.reps)
        print(f"speculative sampling at G = {r['G']}, {r['samples']} samples per dialog: plain sampling call {r['plain_call_ms']:.1f} ms")
        for q in r["per_draft_len"]:
            print(f"  draft_len {q['draft_len']:>2}: one launch on [{q['rows']}, 30522]: unimm_lm_spec_verify = "
                  f"{q['spec_verify_over_sample_rows']:.2f} x unimm_lm_sample_rows ({q['lm_sample_rows_us']:.1f} us, spread "
                  f"{q['sample_rows_spread']:.3f}; {q['mib_read']:.0f} MiB read = x once + xd twice, {q['gb_per_s']:.0f} GB/s; "
                  f"{q['launch_acceptance']:.2f} of the rows accepted); frozen copy as draft: {q['copy_call_ms']:.1f} ms = "
                  f"{q['copy_call_over_plain']:.2f} x the plain call, {q['copy_rounds']} rounds, acceptance {q['copy_acceptance']:.3f}")
    if a.ensemble:
        result["ensemble"] = r = measure_ensemble(model, 80, a.ensemble, a.ensemble_mode, a.reps)
        print(f"ensemble of {r['members']} ({r['mode']}) at G = {r['G']}: one launch on {r['members']} x [{r['rows']}, 30522]: unimm_lm_mix "
              f"{r['lm_mix_us']:.1f} us ({r['lm_mix_mib']:.0f} MiB moved, {r['lm_mix_tb_per_s']:.2f} TB/s; with a cut {r['lm_mix_cut_us']:.1f} us) "
              f"= {r['lm_mix_over_topk']:.2f} x unimm_lm_topk ({r['lm_topk_us']:.1f} us, spread {r['lm_topk_spread']:.3f}); frozen copies as "
              f"partners over the plain call, median of alternating pairs: beams = 1 {r['greedy_ensemble_ratio']:.2f} x "
              f"({r['greedy_call_ms']:.1f} ms, spread {r['greedy_call_spread']:.3f}), 8 samples {r['sample_ensemble_ratio']:.2f} x "
              f"({r['sample_call_ms']:.1f} ms, spread {r['sample_call_spread']:.3f})")
    if a.profile:
        result["kernel_mix_80x4"] = profile()
        for m in result["kernel_mix_80x4"]:
            print(f"  {m['ms_per_step']:8.4f} ms  {m['calls_per_step']:6.2f} x  {m['kernel']}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
