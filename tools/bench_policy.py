"""The policy-gradient row kernels against the likelihood row kernels, and one self-critical step, at the full config.

    python tools/bench_policy.py [--rows 5016] [--pairs 7] [--launches 20] [--no-step] [--G 8] [--N 8] [--shared [--max-answer-len 14]]
                                 [--baseline mean|greedy] [--rollout separate|fused ...] [--kl] [--preference [--reference]] [--distill]

Kernels: unimm_pg_loss_fwd + unimm_pg_loss_bwd against unimm_lm_loss_fwd + unimm_lm_loss_bwd on the SAME fp32 logits
[rows, 30528] (30,522 valid columns; 5,016 rows = the decoded rows of the headline step), in one process as alternating pairs
(lm, pg, lm, pg, ...), each timing `launches` forward + backward pairs between two device events after a warm-up.  Per pair
the tool prints both times and their ratio, then the medians and the run-to-run spread of the likelihood pair (max - min over
its repeats, relative): a ratio further from 1 than that spread is a real difference.  Three objectives: "logp" with beta = 0
(the kernel the bit-equality test compares), "logp" with the entropy bonus, "ratio" clipped with the entropy bonus.  Both pairs
read each logit once per direction (2 x rows x 30522 x 4 bytes) and write rows x 30528 bf16 gradients; the achieved bytes/s
are printed from that count.

Step: one trainer.self_critical_step at G dialogs x N samples (baseline "mean": no greedy pass), split by host clocks around
device synchronisations into sampling (generate_answers), assembly (the reward, self_critical_advantage,
sampled_training_batch and spread: host only, each call clocked) and the train step (forward_backward + optimizer.step);
`other_ms` is what remains of the step's wall time (mode switches, the scheduler, building the constant inputs).
--baseline greedy times the self-critical baseline proper: with --rollout separate the greedy answer is a generate_answers call
of its own (both calls count as sampling), with --rollout fused it is one more slot of the sampling call.  `--rollout separate
fused` times both in one process as alternating pairs (separate, fused, separate, fused, ...; --pairs of them after a warm-up of
each, both steps of a pair with the same seed) and prints the medians of sampling_ms and total_ms, each form's min-to-max spread
over the pairs, the ratios, and whether fused is faster than separate by more than separate's own spread.

--shared (instead of the above): the train-mode step of one sampled batch of G dialogs x N answers in its two forms --
`forward_backward` on G x N full sequences (replicated) and `forward_backward(shared_context=<dialog of each sequence>)`, which
computes each dialog's context and image once -- as alternating pairs in one process after a warm-up: wall time per step between
device synchronisations (medians, every pair's ratio, the replicated step's run-to-run spread), the device kernels each form
launches per step with the mean duration of its text self-attention backward kernel (torch.profiler), and the packed row counts.
--max-answer-len (default 14, the figures of earlier rounds): the longest sampled answer; above 14 the shared step is given
`SharedContext(.., 64)` and runs the two-tile launches when a sampled answer has more than 14 tokens.

--kl (instead of the above): the cost of the KL leash (PolicyObjective.kl_coef + lm_reference).  Kernels: unimm_pg_kl_loss_fwd +
_bwd against unimm_pg_loss_fwd + _bwd on the same logits, the reference row a second buffer of the same size, as alternating
pairs like the kernels above; the KL pair reads twice the bytes per direction, and both byte counts are printed.  Step: one
self_critical_step at G x N (baseline "mean") without a reference and with `reference=frozen_reference(model)`, kl_coef = 0.05, as
alternating pairs with the same seed (--pairs of them after a warm-up of each): medians of the train step and of the whole
step, every pair's ratio and the plain step's min-to-max spread.  The step with a reference adds one inference forward.

--preference (instead of the above): the listwise preference objective on given candidates (policy.PreferenceObjective,
unimm_seq_pref).  The new launch alone, between device events like the kernels above, at 5,016 rows of 64 sequences in 8 groups
and at 5,016 rows of 800 sequences in 8 groups of 100.  Step: the train step (forward_backward + optimizer.step) on G x N
candidates of 1 .. 14 tokens, with --shared on the shared schedule, otherwise on the replicated one, as
alternating pairs after a warm-up of each with the KL-leashed policy-gradient step of --kl on the SAME sequences, schedule and
reference (`lm_advantage`, PolicyObjective(entropy_coef = 0.01, kl_coef = 0.05)): medians, every pair's ratio, the KL step's
min-to-max spread.  --reference: the preference step compares against `frozen_reference(model)` (one more inference forward, as
the KL step always has); without it R = 0.

--distill (instead of the above): token-level knowledge distillation (policy.DistillObjective, unimm_distill_loss_fwd / _bwd).
Kernels: each direction of the distillation pair (tau = 2, alpha = 0.5) on its own, beside the same direction of the likelihood
pair and of the KL pair (LOGP, kl_coef = 0.05) on the same logits and the same second buffer, as alternating launches (lm, kl,
distill; --pairs repeats of --launches launches each): the time, the bytes the direction moves (each row read once; the backward
also writes rows x 30528 bf16) and the bytes/s.  Step: the train step (forward_backward + optimizer.step) on G x N candidates of
1 .. 14 tokens with `lm_objective=DistillObjective()` and `lm_reference=frozen_reference(model)`, with --shared on the shared
schedule, as alternating pairs after a warm-up of each with the KL-leashed policy-gradient step on the SAME sequences, schedule
and frozen model: medians, every pair's ratio, the KL step's min-to-max spread."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG_PATH = os.path.join(ROOT, "unimm_amd", "config", "bert_base_6layer_6conect.json")
V, LD = 30522, 30528


def event_ms(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def kernels(rows, pairs, launches):
    from unimm_amd import lib as L
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn((rows, LD), generator=g) * 3).cuda()
    labels = torch.randint(0, V, (rows,), generator=g).to(torch.int32).cuda()
    weights = torch.ones(rows, dtype=torch.int32, device="cuda")
    adv = torch.randn(rows, generator=g).cuda()
    blogp = (-8.0 + torch.randn(rows, generator=g)).cuda()
    f = lambda: torch.empty(rows, device="cuda")
    rowloss, rownll, lse, ent = f(), f(), f(), f()
    dlog = torch.empty((rows, LD), dtype=torch.bfloat16, device="cuda")
    gvec = torch.ones(1, device="cuda")
    inv = 1.0 / rows

    def lm():
        L.lm_loss_fwd(logits, labels, weights, rowloss, rownll, lse, rows, V)
        L.lm_loss_bwd(logits, labels, weights, lse, gvec, inv, dlog, rows, V)

    def pg(mode, eps, beta):
        def run():
            L.pg_loss_fwd(logits, labels, None, adv, blogp, mode, eps, beta, rowloss, rownll, lse, ent, rows, V)
            L.pg_loss_bwd(logits, labels, None, adv, blogp, mode, eps, beta, lse, ent, gvec, inv, dlog, rows, V)
        return run

    nbytes = 2 * rows * V * 4 + rows * LD * 2
    out = {}
    for name, fn in (("logp", pg(L.PG_LOGP, float("inf"), 0.0)), ("logp_entropy", pg(L.PG_LOGP, float("inf"), 0.01)),
                     ("ratio_clip_entropy", pg(L.PG_RATIO, 0.2, 0.01))):
        t_lm, t_pg = [], []
        for _ in range(pairs):
            t_lm.append(event_ms(lm, launches))
            t_pg.append(event_ms(fn, launches))
        m_lm, m_pg = statistics.median(t_lm), statistics.median(t_pg)
        spread = (max(t_lm) - min(t_lm)) / m_lm
        print(f"{name}: lm fwd+bwd {m_lm * 1e3:.1f} us, pg fwd+bwd {m_pg * 1e3:.1f} us, ratio {m_pg / m_lm:.3f} "
              f"(pairs {[round(p / q, 3) for p, q in zip(t_pg, t_lm)]}; lm spread {spread:.3f}); "
              f"{nbytes / m_lm / 1e9:.2f} / {nbytes / m_pg / 1e9:.2f} TB/s")
        out[name] = dict(lm_us=round(m_lm * 1e3, 1), pg_us=round(m_pg * 1e3, 1), ratio=round(m_pg / m_lm, 4),
                         lm_spread=round(spread, 4), lm_TBps=round(nbytes / m_lm / 1e9, 3), pg_TBps=round(nbytes / m_pg / 1e9, 3))
    return out


def kl_kernels(rows, pairs, launches):
    from unimm_amd import lib as L
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn((rows, LD), generator=g) * 3).cuda()
    ref = (logits + torch.randn((rows, LD), generator=g).cuda() * 0.3).contiguous()
    labels = torch.randint(0, V, (rows,), generator=g).to(torch.int32).cuda()
    adv = torch.randn(rows, generator=g).cuda()
    blogp = (-8.0 + torch.randn(rows, generator=g)).cuda()
    f = lambda: torch.empty(rows, device="cuda")
    rowloss, rownll, lse, ent, kl, ref_lse = f(), f(), f(), f(), f(), f()
    dlog = torch.empty((rows, LD), dtype=torch.bfloat16, device="cuda")
    gvec = torch.ones(1, device="cuda")
    inv = 1.0 / rows

    def pg(mode, eps, beta):
        def run():
            L.pg_loss_fwd(logits, labels, None, adv, blogp, mode, eps, beta, rowloss, rownll, lse, ent, rows, V)
            L.pg_loss_bwd(logits, labels, None, adv, blogp, mode, eps, beta, lse, ent, gvec, inv, dlog, rows, V)
        return run

    def pg_kl(mode, eps, beta, kl_coef):
        def run():
            L.pg_kl_loss_fwd(logits, labels, None, adv, blogp, mode, eps, beta, rowloss, rownll, lse, ent, rows, V, ref, kl_coef, kl, ref_lse)
            L.pg_kl_loss_bwd(logits, labels, None, adv, blogp, mode, eps, beta, lse, ent, gvec, inv, dlog, rows, V, ref, kl_coef, kl,
                             ref_lse)
        return run

    b_pg, b_kl = 2 * rows * V * 4 + rows * LD * 2, 4 * rows * V * 4 + rows * LD * 2
    out = {}
    for name, mode, eps, beta in (("logp_kl", L.PG_LOGP, float("inf"), 0.0), ("logp_entropy_kl", L.PG_LOGP, float("inf"), 0.01),
                                  ("ratio_clip_entropy_kl", L.PG_RATIO, 0.2, 0.01)):
        a, b = pg(mode, eps, beta), pg_kl(mode, eps, beta, 0.05)
        t_pg, t_kl = [], []
        for _ in range(pairs):
            t_pg.append(event_ms(a, launches))
            t_kl.append(event_ms(b, launches))
        m_pg, m_kl = statistics.median(t_pg), statistics.median(t_kl)
        spread = (max(t_pg) - min(t_pg)) / m_pg
        print(f"{name}: pg fwd+bwd {m_pg * 1e3:.1f} us, pg_kl fwd+bwd {m_kl * 1e3:.1f} us, ratio {m_kl / m_pg:.3f} "
              f"(pairs {[round(p / q, 3) for p, q in zip(t_kl, t_pg)]}; pg spread {spread:.3f}); "
              f"{b_pg / m_pg / 1e9:.2f} / {b_kl / m_kl / 1e9:.2f} TB/s")
        out[name] = dict(pg_us=round(m_pg * 1e3, 1), pg_kl_us=round(m_kl * 1e3, 1), ratio=round(m_kl / m_pg, 4),
                         pg_spread=round(spread, 4), pg_TBps=round(b_pg / m_pg / 1e9, 3), pg_kl_TBps=round(b_kl / m_kl / 1e9, 3))
    return out


def kl_step(G, N, pairs):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_generate import dialogs
    from oracle import vilbert_ref as RF
    from unimm_amd import VisualDialogEncoder, policy, trainer
    from unimm_amd.optim import FusedAdamW, WarmupLinearScheduleNonZero, default_language_weights, reference_param_groups
    enc = VisualDialogEncoder(CFG_PATH)
    enc.bert_pretrained.load_state_dict(RF.init_state_dict(RF.make_config(CFG_PATH), seed=5), strict=True)
    enc = enc.cuda()
    ref = policy.frozen_reference(enc)
    groups = reference_param_groups(enc, lr=1e-5, image_lr=1e-5, language_weights=default_language_weights(enc))
    opt = FusedAdamW(groups, enc.bert_pretrained.engine, lr=1e-5)
    sch = WarmupLinearScheduleNonZero(opt, warmup_steps=2, t_total=100, min_lr=1e-6)
    d, c = dialogs(G, seed=3)
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"])
    marks = {}

    def clocked(fn):
        def run(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **kw)
            torch.cuda.synchronize()
            marks["train"] = marks.get("train", 0.0) + (time.perf_counter() - t0) * 1e3
            return r
        return run

    enc.forward_backward, opt.step = clocked(enc.forward_backward), clocked(opt.step)
    reward = lambda tokens, lengths: -lengths.float()
    eng = enc.bert_pretrained.engine

    def one(it, with_ref, seed):
        marks.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), it, reward, samples=N, baseline="mean",
                                         objective=policy.PolicyObjective(entropy_coef=0.01, kl_coef=0.05 if with_ref else 0.0),
                                         temperature=0.8, top_k=50, top_p=0.9, seed=seed, reference=ref if with_ref else None)
        torch.cuda.synchronize()
        row = dict(total_ms=round((time.perf_counter() - t0) * 1e3, 2), train_ms=round(marks["train"], 2), loss=out[0],
                   kl=float(eng.last_lm_kl) if eng.last_lm_kl is not None else None)
        print(f"self_critical_step {it} (G = {G}, N = {N}, reference = {with_ref}): {row}")
        return row

    it = 0
    for _ in range(2):                                       # warm every shape of both forms up
        for w in (False, True):
            it += 1
            one(it, w, 0)
    rows = {False: [], True: []}
    for pair in range(1, pairs + 1):
        for w in (False, True):
            it += 1
            rows[w].append(one(it, w, pair))
    res = dict(G=G, N=N, pairs=pairs)
    for key in ("train_ms", "total_ms"):
        med = {w: statistics.median(x[key] for x in rows[w]) for w in (False, True)}
        res[key] = dict(plain=med[False], with_reference=med[True], ratio=round(med[True] / med[False], 4),
                        pair_ratios=[round(y[key] / x[key], 3) for x, y in zip(rows[False], rows[True])],
                        plain_spread=round(max(x[key] for x in rows[False]) - min(x[key] for x in rows[False]), 2))
    res["mean_kl"] = [x["kl"] for x in rows[True]]
    print(f"KL leash, step: {res}")
    return res


def pref_kernels(rows, pairs, launches):
    from unimm_amd import lib as L
    g = torch.Generator().manual_seed(0)
    out = {}
    for name, B, groups in (("64_sequences_8_groups", 64, 8), ("800_sequences_8_groups_of_100", 800, 8)):
        rownll = (torch.rand(rows, generator=g) * 6).cuda()
        ref = (torch.rand(rows, generator=g) * 6).cuda()
        row_seq = (torch.arange(rows) % B).to(torch.int32)[torch.randperm(rows, generator=g)].cuda()
        seq_group = (torch.arange(B) % groups).to(torch.int32).cuda()
        weight = torch.softmax(torch.randn(groups, B // groups, generator=g), 1).t().reshape(-1).contiguous().cuda()
        adv, score, prob = torch.empty(rows, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        gl, ai = torch.empty(groups, device="cuda"), torch.empty(1, device="cuda")
        ws = torch.empty(L.PREF_WS_ITEM_BYTES * (B + groups), dtype=torch.uint8, device="cuda")
        fn = lambda: L.seq_pref(rownll, ref, row_seq, rows, seq_group, weight, groups, 0.1, False, adv, score, prob, gl, ai,
                                workspace=ws)
        t = [event_ms(fn, launches) for _ in range(pairs)]
        m = statistics.median(t)
        print(f"unimm_seq_pref, {rows} rows, {name}: {m * 1e3:.1f} us per call (three launches; min {min(t) * 1e3:.1f}, max "
              f"{max(t) * 1e3:.1f} over {pairs} repeats of {launches} calls)")
        out[name] = dict(rows=rows, sequences=B, groups=groups, us=round(m * 1e3, 1), min_us=round(min(t) * 1e3, 1),
                         max_us=round(max(t) * 1e3, 1))
    return out


def pref_step(G, N, pairs, with_reference, share):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_generate import dialogs
    from oracle import vilbert_ref as RF
    from unimm_amd import SharedContext, VisualDialogEncoder, policy
    from unimm_amd.optim import FusedAdamW, default_language_weights, reference_param_groups
    enc = VisualDialogEncoder(CFG_PATH)
    enc.bert_pretrained.load_state_dict(RF.init_state_dict(RF.make_config(CFG_PATH), seed=5), strict=True)
    enc = enc.cuda()
    ref = policy.frozen_reference(enc)
    eng = enc.bert_pretrained.engine
    groups = reference_param_groups(enc, lr=1e-5, image_lr=1e-5, language_weights=default_language_weights(enc))
    opt = FusedAdamW(groups, eng, lr=1e-5)
    d, c = dialogs(G, seed=3)
    T, R, C = d["input_ids"].shape[1], d["image_feat"].shape[1], eng.cfg.v_target_size
    rng = np.random.default_rng(1)
    lengths = torch.from_numpy(rng.integers(2, 16, (G, N)))                       # 1 .. 14 tokens and the [SEP]
    tokens = torch.from_numpy(rng.integers(1000, 20000, (G, N, 15)))
    sb = policy.candidate_training_batch(d["input_ids"], d["token_type_ids"], d["position_ids"], c, tokens, lengths, T)
    K = sb.input_ids.shape[0]
    w = policy.relevance_targets(torch.from_numpy(rng.integers(0, 5, (G, N)) * 0.5))
    tg = policy.PreferenceTargets(sb.image_index, w.reshape(-1)[sb.kept])
    label = torch.zeros((K, R), dtype=torch.int64)
    label[:, 0] = 1
    kw = dict(token_type_ids=sb.token_type_ids, token_position_ids=sb.position_ids, attention_mask=sb.attention_mask,
              masked_lm_labels=sb.masked_lm_labels, next_sentence_label=torch.zeros(K, dtype=torch.int64),
              image_attention_mask=d["image_attention_mask"][sb.image_index.to(d["image_attention_mask"].device)],
              image_label=label, image_target=torch.full((G, R, C), 1.0 / C), image_index=sb.image_index,
              **(dict(shared_context=SharedContext(sb.image_index, 64)) if share else {}))
    forms = dict(
        kl=dict(lm_advantage=policy.spread(torch.from_numpy(rng.standard_normal((G, N))), sb),
                lm_objective=policy.PolicyObjective(entropy_coef=0.01, kl_coef=0.05), lm_reference=ref),
        preference=dict(lm_preference=tg, lm_objective=policy.PreferenceObjective(), lm_reference=ref if with_reference else None))
    enc.train()

    def wall_ms(form, n=3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = enc.forward_backward(sb.input_ids, d["image_feat"], d["image_loc"], (1.0, 0.0, 0.0), **kw, **forms[form])[1]
            opt.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, float(loss)

    for form in forms:                                       # warm every shape of both forms up
        wall_ms(form, 2)
    t = {form: [] for form in forms}
    loss = {}
    for _ in range(pairs):
        for form in forms:
            ms, loss[form] = wall_ms(form)
            t[form].append(ms)
    med = {form: statistics.median(v) for form, v in t.items()}
    res = dict(G=G, N=N, sequences=K, rows=int(sb.copy_rows.sum()), shared=bool(share), reference=bool(with_reference), pairs=pairs,
               kl_ms=round(med["kl"], 3), preference_ms=round(med["preference"], 3), ratio=round(med["preference"] / med["kl"], 4),
               pair_ratios=[round(a / b, 3) for a, b in zip(t["preference"], t["kl"])],
               kl_spread=round((max(t["kl"]) - min(t["kl"])) / med["kl"], 4), loss=loss)
    print(f"preference step beside the KL step (G = {G}, N = {N}): {res}")
    return res


def distill_kernels(rows, pairs, launches):
    from unimm_amd import lib as L
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn((rows, LD), generator=g) * 3).cuda()
    ref = (logits + torch.randn((rows, LD), generator=g).cuda() * 0.3).contiguous()
    labels = torch.randint(0, V, (rows,), generator=g).to(torch.int32).cuda()
    weights = torch.ones(rows, dtype=torch.int32, device="cuda")
    adv = torch.randn(rows, generator=g).cuda()
    f = lambda: torch.empty(rows, device="cuda")
    rowloss, rownll, lse, ent, kl, ref_lse, lse_t, ref_lse_t, kd = (f() for _ in range(9))
    dlog = torch.empty((rows, LD), dtype=torch.bfloat16, device="cuda")
    gvec = torch.ones(1, device="cuda")
    inv, inf = 1.0 / rows, float("inf")
    tau, alpha = 2.0, 0.5
    fns = dict(
        lm_fwd=lambda: L.lm_loss_fwd(logits, labels, weights, rowloss, rownll, lse, rows, V),
        lm_bwd=lambda: L.lm_loss_bwd(logits, labels, weights, lse, gvec, inv, dlog, rows, V),
        kl_fwd=lambda: L.pg_kl_loss_fwd(logits, labels, None, adv, None, L.PG_LOGP, inf, 0.0, rowloss, rownll, lse, ent, rows, V, ref,
                                        0.05, kl, ref_lse),
        kl_bwd=lambda: L.pg_kl_loss_bwd(logits, labels, None, adv, None, L.PG_LOGP, inf, 0.0, lse, ent, gvec, inv, dlog, rows, V, ref,
                                        0.05, kl, ref_lse),
        distill_fwd=lambda: L.distill_loss_fwd(logits, labels, weights, ref, tau, alpha, rowloss, rownll, lse, lse_t, ref_lse_t, kd,
                                               rows, V),
        distill_bwd=lambda: L.distill_loss_bwd(logits, labels, weights, ref, tau, alpha, lse, lse_t, ref_lse_t, gvec, inv, dlog, rows, V))
    for name in ("lm", "kl", "distill"):                     # every backward reads what its own forward left
        fns[name + "_fwd"]()
    one, two = rows * V * 4, 2 * rows * V * 4
    nbytes = dict(lm_fwd=one, lm_bwd=one + rows * LD * 2, kl_fwd=two, kl_bwd=two + rows * LD * 2, distill_fwd=two,
                  distill_bwd=two + rows * LD * 2)
    t = {k: [] for k in fns}
    for _ in range(pairs):                                   # alternating: lm, kl, distill, each direction on its own
        for d in ("fwd", "bwd"):
            for name in ("lm", "kl", "distill"):
                fns[name + "_fwd"]()
                t[f"{name}_{d}"].append(event_ms(fns[f"{name}_{d}"], launches))
    out = dict(rows=rows, tau=tau, alpha=alpha)
    for k, v in t.items():
        m = statistics.median(v)
        out[k] = dict(us=round(m * 1e3, 1), min_us=round(min(v) * 1e3, 1), max_us=round(max(v) * 1e3, 1), bytes=nbytes[k],
                      TBps=round(nbytes[k] / m / 1e9, 3))
        print(f"{k}: {m * 1e3:.1f} us (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f} over {pairs} repeats of {launches} launches), "
              f"{nbytes[k] / 1e6:.1f} MB, {nbytes[k] / m / 1e9:.2f} TB/s")
    for name in ("lm", "kl", "distill"):
        us = out[name + "_fwd"]["us"] + out[name + "_bwd"]["us"]
        b = nbytes[name + "_fwd"] + nbytes[name + "_bwd"]
        out[name + "_pair"] = dict(us=round(us, 1), TBps=round(b / us / 1e6, 3))
        print(f"{name} fwd+bwd: {us:.1f} us, {b / us / 1e6:.2f} TB/s")
    out["distill_over_kl"] = round(out["distill_pair"]["us"] / out["kl_pair"]["us"], 4)
    return out


def distill_step(G, N, pairs, share):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_generate import dialogs
    from oracle import vilbert_ref as RF
    from unimm_amd import SharedContext, VisualDialogEncoder, policy
    from unimm_amd.optim import FusedAdamW, default_language_weights, reference_param_groups
    enc = VisualDialogEncoder(CFG_PATH)
    enc.bert_pretrained.load_state_dict(RF.init_state_dict(RF.make_config(CFG_PATH), seed=5), strict=True)
    enc = enc.cuda()
    ref = policy.frozen_reference(enc)
    eng = enc.bert_pretrained.engine
    groups = reference_param_groups(enc, lr=1e-5, image_lr=1e-5, language_weights=default_language_weights(enc))
    opt = FusedAdamW(groups, eng, lr=1e-5)
    d, c = dialogs(G, seed=3)
    T, R, C = d["input_ids"].shape[1], d["image_feat"].shape[1], eng.cfg.v_target_size
    rng = np.random.default_rng(1)
    lengths = torch.from_numpy(rng.integers(2, 16, (G, N)))                       # 1 .. 14 tokens and the [SEP]
    tokens = torch.from_numpy(rng.integers(1000, 20000, (G, N, 15)))
    sb = policy.candidate_training_batch(d["input_ids"], d["token_type_ids"], d["position_ids"], c, tokens, lengths, T)
    K = sb.input_ids.shape[0]
    label = torch.zeros((K, R), dtype=torch.int64)
    label[:, 0] = 1
    kw = dict(token_type_ids=sb.token_type_ids, token_position_ids=sb.position_ids, attention_mask=sb.attention_mask,
              masked_lm_labels=sb.masked_lm_labels, next_sentence_label=torch.zeros(K, dtype=torch.int64),
              image_attention_mask=d["image_attention_mask"][sb.image_index.to(d["image_attention_mask"].device)],
              image_label=label, image_target=torch.full((G, R, C), 1.0 / C), image_index=sb.image_index,
              **(dict(shared_context=SharedContext(sb.image_index, 64)) if share else {}))
    forms = dict(
        kl=dict(lm_advantage=policy.spread(torch.from_numpy(rng.standard_normal((G, N))), sb),
                lm_objective=policy.PolicyObjective(entropy_coef=0.01, kl_coef=0.05), lm_reference=ref),
        distill=dict(lm_objective=policy.DistillObjective(2.0, 0.5), lm_reference=ref))
    enc.train()

    def wall_ms(form, n=3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = enc.forward_backward(sb.input_ids, d["image_feat"], d["image_loc"], (1.0, 0.0, 0.0), **kw, **forms[form])[1]
            opt.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, float(loss)

    for form in forms:                                       # warm every shape of both forms up
        wall_ms(form, 2)
    t = {form: [] for form in forms}
    loss = {}
    for _ in range(pairs):
        for form in forms:
            ms, loss[form] = wall_ms(form)
            t[form].append(ms)
    med = {form: statistics.median(v) for form, v in t.items()}
    res = dict(G=G, N=N, sequences=K, rows=int(sb.copy_rows.sum()), shared=bool(share), pairs=pairs, kl_ms=round(med["kl"], 3),
               distill_ms=round(med["distill"], 3), ratio=round(med["distill"] / med["kl"], 4),
               pair_ratios=[round(a / b, 3) for a, b in zip(t["distill"], t["kl"])],
               kl_spread=round((max(t["kl"]) - min(t["kl"])) / med["kl"], 4), loss=loss,
               mean_kd=float(eng.last_lm_distill) if eng.last_lm_distill is not None else None)
    print(f"distillation step beside the KL step (G = {G}, N = {N}): {res}")
    return res


def step(G, N, baseline="mean", rollouts=("separate",), pairs=7):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_generate import dialogs
    from oracle import vilbert_ref as RF
    from unimm_amd import VisualDialogEncoder, policy, trainer
    from unimm_amd.optim import FusedAdamW, WarmupLinearScheduleNonZero, default_language_weights, reference_param_groups
    enc = VisualDialogEncoder(CFG_PATH)
    enc.bert_pretrained.load_state_dict(RF.init_state_dict(RF.make_config(CFG_PATH), seed=5), strict=True)
    enc = enc.cuda()
    groups = reference_param_groups(enc, lr=1e-5, image_lr=1e-5, language_weights=default_language_weights(enc))
    opt = FusedAdamW(groups, enc.bert_pretrained.engine, lr=1e-5)
    sch = WarmupLinearScheduleNonZero(opt, warmup_steps=2, t_total=100, min_lr=1e-6)
    d, c = dialogs(G, seed=3)
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"])
    marks = {}
    real_gen, real_fb = enc.generate_answers, enc.forward_backward

    def clocked(name, fn):
        def run(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **kw)
            torch.cuda.synchronize()
            marks[name] = marks.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            if name == "sampling":                           # decode steps walked: the longest answer of every call
                marks["decode_steps"] = marks.get("decode_steps", 0) + max(
                    int(x.lengths.max()) for x in (r, getattr(r, "greedy", None)) if x is not None)
            return r
        return run

    enc.generate_answers, enc.forward_backward = clocked("sampling", real_gen), clocked("train", real_fb)
    opt.step = clocked("train", opt.step)
    for name in ("sampled_training_batch", "spread", "self_critical_advantage"):       # the names the step calls
        setattr(trainer, name, clocked("assembly", getattr(policy, name)))
    reward = clocked("assembly", lambda tokens, lengths: -lengths.float())
    def one(it, rollout, seed=None):
        marks.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), it, reward, samples=N, baseline=baseline,
                                         objective=policy.PolicyObjective(entropy_coef=0.01), temperature=0.8, top_k=50, top_p=0.9,
                                         seed=seed, **(dict(rollout=rollout) if rollout != "separate" else {}))
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        row = dict(total_ms=round(total, 2), sampling_ms=round(marks["sampling"], 2), assembly_ms=round(marks["assembly"], 2),
                   train_ms=round(marks["train"], 2),
                   other_ms=round(total - marks["sampling"] - marks["assembly"] - marks["train"], 2), loss=out[0])
        if baseline != "mean" or rollout != "separate":
            row.update(baseline=baseline, rollout=rollout, decode_steps=marks["decode_steps"])
        print(f"self_critical_step {it} (G = {G}, N = {N}): {row}")
        return row

    if len(rollouts) == 1:
        return [one(it, rollouts[0]) for it in range(1, 5)]   # the first iterations warm every shape up
    it = 0
    for _ in range(2):                                       # warm every shape of both forms up
        for r in rollouts:
            it += 1
            one(it, r, seed=0)
    rows = {r: [] for r in rollouts}
    for pair in range(1, pairs + 1):
        for r in rollouts:
            it += 1
            rows[r].append(one(it, r, seed=pair))
    res = dict(G=G, N=N, baseline=baseline, pairs=pairs)
    for key in ("sampling_ms", "total_ms"):
        med = {r: statistics.median(x[key] for x in rows[r]) for r in rollouts}
        spread = {r: round(max(x[key] for x in rows[r]) - min(x[key] for x in rows[r]), 2) for r in rollouts}
        a, b = rollouts
        res[key] = dict(median=med, spread=spread, ratio=round(med[b] / med[a], 4),
                        pair_ratios=[round(y[key] / x[key], 3) for x, y in zip(rows[a], rows[b])],
                        second_faster_by_more_than_first_spread=bool(med[a] - med[b] > spread[a]))
    res["decode_steps"] = {r: [x["decode_steps"] for x in rows[r]] for r in rollouts}
    print(f"rollouts {rollouts}: {res}")
    return dict(summary=res, rows=rows)


def shared(G, N, pairs, max_answer_len=14):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_generate import dialogs
    from oracle import vilbert_ref as RF
    from unimm_amd import VisualDialogEncoder, policy
    enc = VisualDialogEncoder(CFG_PATH)
    enc.bert_pretrained.load_state_dict(RF.init_state_dict(RF.make_config(CFG_PATH), seed=5), strict=True)
    enc = enc.cuda()
    eng = enc.bert_pretrained.engine
    d, c = dialogs(G, seed=3)
    T, R, C = d["input_ids"].shape[1], d["image_feat"].shape[1], eng.cfg.v_target_size
    enc.eval()
    # (the default, answers of at most 14 tokens: 1 + 2 (14 + 1) = 31 private rows, the shared step's one query tile and the
    # figures of earlier rounds; up to 30: two tiles, through SharedContext(.., 64))
    from unimm_amd import SharedContext
    ans = enc.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, token_type_ids=d["token_type_ids"],
                               position_ids=d["position_ids"], image_attention_mask=d["image_attention_mask"],
                               samples=N, temperature=0.8, top_k=50, top_p=0.9, seed=1, max_answer_len=max_answer_len)
    sb = policy.sampled_training_batch(d["input_ids"], d["token_type_ids"], d["position_ids"], c, ans, T)
    K = sb.input_ids.shape[0]
    adv = policy.self_critical_advantage(-ans.lengths.cpu().float(), "mean" if N > 1 else None)
    label = torch.zeros((K, R), dtype=torch.int64)
    label[:, 0] = 1
    kw = dict(token_type_ids=sb.token_type_ids, token_position_ids=sb.position_ids, attention_mask=sb.attention_mask,
              masked_lm_labels=sb.masked_lm_labels, next_sentence_label=torch.zeros(K, dtype=torch.int64),
              image_attention_mask=d["image_attention_mask"][sb.image_index.to(d["image_attention_mask"].device)],
              image_label=label, image_target=torch.full((G, R, C), 1.0 / C), image_index=sb.image_index,
              lm_advantage=policy.spread(adv, sb), lm_objective=policy.PolicyObjective(entropy_coef=0.01))
    enc.train()
    ctx_arg = sb.image_index if max_answer_len <= 14 else SharedContext(sb.image_index, 64)

    def one(share):
        eng.arena.zero_grads()
        return enc.forward_backward(sb.input_ids, d["image_feat"], d["image_loc"], (1.0, 0.0, 0.0),
                                    **kw, **(dict(shared_context=ctx_arg) if share else {}))[1]

    def wall_ms(share, n=3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            one(share)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def launches(share):
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                one(share)
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
            attn = {}                                          # the text self-attention backward kernels: launches, mean us
            for e in ev:
                for key in ("attn_spliced_bwd", "attn_spliced_wide_bwd", "attn_bwd_fused"):
                    if key in e.name:
                        t = getattr(e, "device_time", None)
                        a = attn.setdefault(key, [0, 0.0])
                        a[0] += 1
                        a[1] += float(t if t is not None else e.cuda_time)
            return dict(launches=len(ev), **{k: dict(launches=v[0], mean_us=round(v[1] / v[0], 1)) for k, v in attn.items()})
        except Exception as e:                                 # the counts are a report, not a result
            return f"unavailable ({type(e).__name__}: {e})"

    losses = {s_: float(one(s_)) for s_ in (False, True)}
    for s_ in (False, True):                                   # warm every shape up
        wall_ms(s_, 2)
    t_rep, t_sh = [], []
    for _ in range(pairs):
        t_rep.append(wall_ms(False))
        t_sh.append(wall_ms(True))
    m_rep, m_sh = statistics.median(t_rep), statistics.median(t_sh)
    n_ans = sb.attention_mask.answer.astype(np.int64)
    ctx = (sb.attention_mask.length.astype(np.int64) - n_ans)
    first = np.unique(sb.image_index.numpy(), return_index=True)[1]
    res = dict(G=G, N=N, max_answer_len=max_answer_len, longest_answer=int(n_ans.max()) - 1, sequences=K, replicated_ms=round(m_rep, 3), shared_ms=round(m_sh, 3), ratio=round(m_sh / m_rep, 4),
               pair_ratios=[round(a / b, 3) for a, b in zip(t_sh, t_rep)], replicated_spread=round((max(t_rep) - min(t_rep)) / m_rep, 4),
               text_rows_replicated=int((ctx + 2 * n_ans).sum()), text_rows_shared=int((ctx[first] - 1).sum() + (1 + 2 * n_ans).sum()),
               region_rows_replicated=K * R, region_rows_shared=len(first) * R,
               launches_replicated=launches(False), launches_shared=launches(True), loss_replicated=losses[False], loss_shared=losses[True])
    print(f"shared-context step (G = {G}, N = {N}): {res}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5016)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--shared", action="store_true", help="time the shared-context train step beside the replicated one")
    ap.add_argument("--max-answer-len", type=int, default=14,
                    help="--shared: longest sampled answer (above 14 the step takes SharedContext(.., 64) and may run the two-tile launches)")
    ap.add_argument("--baseline", choices=("mean", "greedy"), default="mean", help="the step's baseline (greedy: with the greedy pass)")
    ap.add_argument("--rollout", choices=("separate", "fused"), nargs="+", default=["separate"],
                    help="how the greedy baseline is decoded; both values: alternating pairs in one process")
    ap.add_argument("--kl", action="store_true", help="time the KL-regularised row kernels and the step with a frozen reference")
    ap.add_argument("--preference", action="store_true", help="time unimm_seq_pref and the preference train step beside the KL step")
    ap.add_argument("--reference", action="store_true", help="--preference: the step compares against a frozen reference")
    ap.add_argument("--distill", action="store_true", help="time the distillation row kernels and the train step with a teacher")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy.py measures on the GPU: no device found")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if a.preference:
        result = dict(rows=a.rows, pref_kernels=pref_kernels(a.rows, a.pairs, a.launches))
        if not a.no_step:
            result["pref_step"] = pref_step(a.G, a.N, a.pairs, a.reference, a.shared)
        print(json.dumps(result))
        return
    if a.distill:
        result = dict(rows=a.rows, distill_kernels=distill_kernels(a.rows, a.pairs, a.launches))
        if not a.no_step:
            result["distill_step"] = distill_step(a.G, a.N, a.pairs, a.shared)
        print(json.dumps(result))
        return
    if a.kl:
        result = dict(rows=a.rows, kl_kernels=kl_kernels(a.rows, a.pairs, a.launches))
        if not a.no_step:
            result["kl_step"] = kl_step(a.G, a.N, a.pairs)
        print(json.dumps(result))
        return
    if a.shared:
        print(json.dumps(dict(shared=shared(a.G, a.N, a.pairs, a.max_answer_len))))
        return
    result = dict(rows=a.rows, kernels=kernels(a.rows, a.pairs, a.launches))
    if not a.no_step:
        if len(a.rollout) > 2 or len(set(a.rollout)) != len(a.rollout):
            raise SystemExit("--rollout takes separate, fused, or both once each")
        if "fused" in a.rollout and a.baseline != "greedy":
            raise SystemExit("--rollout fused needs --baseline greedy")
        result["step"] = step(a.G, a.N, a.baseline, tuple(a.rollout), a.pairs)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
