"""generate_answers with the history rules (no_repeat_ngram_size, repetition_penalty, repeat_scope) on the GPU, on the tiny model
and dialogs of tests/test_gpu_generate.py / tests/test_gpu_generate_rollout.py: answers that must be permutations whatever the
weights are, scores that stay `sequence_log_likelihood` of the completed sequence under the n-gram rule, the dialog scope, the
greedy slot against beams = 1 under a penalty, step_logq against step_logp, which kernels a call launches, and one
self_critical_step under the rule on both rollouts."""
import math

import numpy as np
import pytest
import torch

from tests import constrain_ref as CR
from tests.test_gpu_generate import SEP, answers_of, completed, gen_kwargs, tiny  # noqa: F401
from tests.test_gpu_generate_rollout import G_TINY, MAXLEN, T_TINY, flat_greedy, generate, limit_of, tiny_dialogs
from tests.test_gpu_generate_sample import flat

pytestmark = pytest.mark.gpu
V_TINY = 1000
DEFAULT_BANNED = (0, 101, 103)


def all_answers(res):
    """[(g, j, answer tokens without [SEP])] of every returned hypothesis, each ending in its one [SEP]."""
    out = []
    for g in range(res.lengths.shape[0]):
        for j in range(res.lengths.shape[1]):
            ans, n = answers_of(res, g, j)
            assert n >= 1 and int(res.tokens[g, j, n - 1]) == SEP and SEP not in ans and (res.tokens[g, j, n:] == 0).all()
            out.append((g, j, ans))
    return out


@pytest.mark.parametrize("kw", [dict(beams=1), dict(beams=3), dict(samples=4, seed=3)], ids=["beams1", "beams3", "samples4"])
def test_four_free_ids_give_permutations(tiny, kw):
    """Every id but four and [SEP] banned, unigrams never repeated, at least four tokens: each answer is a permutation of the
    four ids followed by [SEP], whatever the weights are."""
    model, _, _ = tiny
    d, c, _ = tiny_dialogs()
    free = [200, 300, 400, 500]
    banned = tuple(i for i in range(V_TINY) if i not in free and i != SEP)
    res = generate(model, d, c, banned_tokens=banned, no_repeat_ngram_size=1, min_answer_len=4, max_answer_len=8, **kw)
    answers = all_answers(res)
    assert len(answers) == G_TINY * (kw.get("samples") or kw["beams"])
    for g, j, ans in answers:
        assert sorted(ans) == free, (g, j, ans)
    assert torch.isfinite(res.logp).all() and (res.lengths == 5).all()


@pytest.mark.parametrize("kw", [dict(beams=3), dict(samples=4, seed=3)], ids=["beams3", "samples4"])
def test_no_repeated_bigram_and_scores_stay_the_sequence_log_likelihood(tiny, kw):
    """no_repeat_ngram_size = 2 on the whole vocabulary: no answer repeats a bigram, and every logp equals
    sequence_log_likelihood of the completed sequence within 2e-3 of the largest |value| (the bound of
    test_full_config_scores_equal_sequence_log_likelihood for the same comparison)."""
    model, _, _ = tiny
    d, c, utts = tiny_dialogs()
    res = generate(model, d, c, no_repeat_ngram_size=2, **kw)
    answers = all_answers(res)
    for g, j, ans in answers:
        assert not CR.repeats_ngram(ans, 2), (g, j, ans)
        assert not set(ans) & set(DEFAULT_BANNED)
    gs = [g for g, _, _ in answers]
    seq, _ = completed([utts[g] for g in gs], [a for _, _, a in answers], T_TINY)
    dev = "cuda"
    want, _ = model.sequence_log_likelihood(seq["tokens"].to(dev), d["image_feat"][gs].to(dev), d["image_loc"][gs].to(dev),
                                            seq["labels"].to(dev), token_type_ids=seq["segments"].to(dev),
                                            position_ids=seq["positions"].to(dev), attention_mask=seq["txt_attention_mask"].to(dev),
                                            co_attention_mask=seq["co_attention_mask"].to(dev),
                                            image_attention_mask=d["image_attention_mask"][gs].to(dev))
    got = torch.stack([res.scores[g, j] for g, j, _ in answers]).cpu()
    want = want.cpu()
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"\nno_repeat_ngram_size = 2, {kw}: scores {float(got.min()):.3f} .. {float(got.max()):.3f}, "
          f"|generated - sequence_log_likelihood| {err:.3e} ({err / scale:.2e} of scale)")
    assert err <= 2e-3 * scale
    # the rule binds on this model: without it some answer repeats a bigram
    plain = generate(model, d, c, **kw)
    print(f"without the rule {sum(CR.repeats_ngram(a, 2) for _, _, a in all_answers(plain))} of {len(answers)} answers repeat a bigram")


@pytest.mark.parametrize("kw", [dict(beams=2), dict(samples=3, seed=5, greedy=True)], ids=["beams2", "samples3"])
def test_dialog_scope_keeps_context_tokens_out(tiny, kw):
    model, _, _ = tiny
    d, c, _ = tiny_dialogs()
    res = generate(model, d, c, no_repeat_ngram_size=1, repeat_scope="dialog", **kw)
    for out in (res, res.greedy) if res.greedy is not None else (res,):
        for g, j, ans in all_answers(out):
            context = set(d["input_ids"][g, 1:int(c[g])].tolist())
            assert ans and not set(ans) & context and len(set(ans)) == len(ans), (g, j, ans)


def oracle_logits(ocfg, sd, d, g, utts, prefix):
    """The oracle's fp64 logits of the copy row after `prefix` (teacher-forced), for dialog g."""
    from oracle import vilbert_ref as R
    seq, Ls = completed([utts[g]], [prefix], T_TINY)
    with torch.no_grad():
        out = R.forward(sd, ocfg, seq["tokens"], d["image_feat"][[g]], d["image_loc"][[g]], token_type_ids=seq["segments"],
                        position_ids=seq["positions"], attention_mask=seq["txt_attention_mask"],
                        image_attention_mask=d["image_attention_mask"][[g]], co_attention_mask=seq["co_attention_mask"])
    return out["pred_t"][0, Ls[0] + len(prefix)].double()


def test_greedy_slot_and_beams_1_agree_under_a_penalty(tiny):
    """samples = 3, greedy = True, repetition_penalty = 1.3: the greedy slot decodes what beams = 1 decodes under the same penalty.
    Tokens may first differ only where the oracle's top two PENALISED logits (after the step rules) are within 0.05, the
    allowance of test_tiny_batch_invariance_and_no_side_effects; at least 5 of the 6 dialogs agree."""
    model, ocfg, sd = tiny
    d, c, utts = tiny_dialogs()
    r = 1.3
    fused = generate(model, d, c, samples=3, greedy=True, repetition_penalty=r, seed=3)
    alone = generate(model, d, c, beams=1, repetition_penalty=r)
    plain = generate(model, d, c, beams=1)
    flat(fused), flat_greedy(fused.greedy), flat_greedy(alone)
    agree = 0
    for g in range(G_TINY):
        a = answers_of(fused.greedy, g, 0)[0] + [SEP]
        b = answers_of(alone, g, 0)[0] + [SEP]
        k = next((i for i, (p, q) in enumerate(zip(a, b)) if p != q), None)
        if k is None:
            assert a == b
            agree += 1
            u, v = fused.greedy.step_logp[g, 0], alone.step_logp[g, 0]
            assert ((u - v).abs() <= 1e-3 * v.abs() + 1e-5).all(), (g, u, v)
            continue
        x = oracle_logits(ocfg, sd, d, g, utts, a[:k]).float().numpy()
        xp = torch.from_numpy(CR.penalised_row(x, a[:k], None, np.float32(r), np.float32(1.0 / float(np.float32(r))))).double()
        xp[list(DEFAULT_BANNED) + ([SEP] if k < 1 else [])] = -math.inf       # min_answer_len = 1
        if k >= limit_of(c, g):
            xp[[i for i in range(V_TINY) if i != SEP]] = -math.inf
        top2 = torch.topk(xp, 2).values
        assert float(top2[0] - top2[1]) <= 0.05, (g, k, top2)
    print(f"\ngreedy slot against beams = 1 under repetition_penalty = {r}: {agree} of {G_TINY} dialogs agree")
    assert agree >= 5
    # reported values are raw log p: the summed logp of a penalised greedy answer is that of its tokens
    assert torch.isfinite(alone.logp).all() and torch.allclose(alone.logp, alone.step_logp.sum(-1), rtol=1e-5, atol=1e-5)
    print(f"the penalty changes {int((alone.tokens != plain.tokens).any(-1).sum())} of {G_TINY} greedy answers")


def test_step_logq_reports_the_penalised_distribution(tiny):
    model, _, _ = tiny
    d, c, _ = tiny_dialogs()
    res = generate(model, d, c, samples=4, repetition_penalty=1.3, seed=3)
    rows = flat(res)
    differ = 0
    for g, j, _, n in rows:
        p, q = res.step_logp[g, j, :n], res.step_logq[g, j, :n]
        assert torch.isfinite(p).all() and torch.isfinite(q).all()
        differ += int((p != q).any())
    plain = generate(model, d, c, samples=4, seed=3)
    # step 0 has no history: the first draw's logq equals logp as without the penalty; later steps see the penalty
    assert torch.equal(res.step_logq[:, :, 0], plain.step_logq[:, :, 0]) and torch.equal(res.tokens[:, :, 0], plain.tokens[:, :, 0])
    later = sum(int((res.step_logp[g, j, 1:n] != res.step_logq[g, j, 1:n]).any()) for g, j, _, n in rows)
    print(f"\nrepetition_penalty = 1.3: step_logq != step_logp after step 0 on {later} of {len(rows)} sampled answers")
    assert differ > 0 and later > 0


def test_which_kernels_a_constrained_call_launches(tiny, monkeypatch):
    from unimm_amd import generation as GN
    model, _, _ = tiny
    d, c, _ = tiny_dialogs()
    names = ("lm_topk", "lm_sample", "lm_sample_rows", "lm_topk_hist", "lm_sample_hist")
    counts = dict.fromkeys(names, 0)
    for name in names:
        def counted(*a, _f=getattr(GN.L, name), _n=name, **kw):
            counts[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(GN.L, name, counted)

    def launched():
        got = {k: v for k, v in counts.items() if v}
        counts.update(dict.fromkeys(names, 0))
        return got

    base_beam = generate(model, d, c, beams=3)
    assert set(launched()) == {"lm_topk"}
    base_samp = generate(model, d, c, samples=3, seed=3, top_k=20)
    assert set(launched()) == {"lm_sample"}
    for kw in (dict(no_repeat_ngram_size=2), dict(no_repeat_ngram_size=1, repeat_scope="dialog"), dict(repetition_penalty=1.2)):
        generate(model, d, c, beams=1 if "repetition_penalty" in kw else 3, **kw)
        got = launched()
        assert set(got) == {"lm_topk_hist"} and got["lm_topk_hist"] >= 2, (kw, got)
        generate(model, d, c, samples=3, seed=3, top_k=20, **kw)
        got = launched()
        assert set(got) == {"lm_sample_hist"} and got["lm_sample_hist"] >= 2, (kw, got)
        generate(model, d, c, samples=3, seed=3, greedy=True, **kw)
        assert set(launched()) == {"lm_sample_hist"}
    # the keywords at their `off` values: the kernels of the call without them, and its bits
    off = dict(no_repeat_ngram_size=0, repetition_penalty=1.0, repeat_scope="dialog")
    beam = generate(model, d, c, beams=3, **off)
    assert set(launched()) == {"lm_topk"}
    samp = generate(model, d, c, samples=3, seed=3, top_k=20, **off)
    assert set(launched()) == {"lm_sample"}
    for a, b in ((beam, base_beam), (samp, base_samp)):
        for f in ("tokens", "lengths", "scores", "logp", "step_logp", "step_logq"):
            u, v = getattr(a, f), getattr(b, f)
            assert (u is None and v is None) or torch.equal(u, v), f


@pytest.mark.parametrize("rollout", ["separate", "fused"])
def test_self_critical_step_under_the_ngram_rule(rollout):
    from tests.test_gpu_generate import make_dialogs
    from tests.test_gpu_policy_model import _encoder
    from unimm_amd import trainer
    enc, opt, sch = _encoder()
    d, c, _ = make_dialogs(4, T_TINY, V_TINY, 37, 192, seed=8, cmin=8, cmax=40)
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"])
    calls, real = [], enc.generate_answers

    def counted(*a, **kw):
        calls.append(dict(kw, result=real(*a, **kw)))
        return calls[-1]["result"]

    enc.generate_answers = counted
    reward = lambda tokens, lengths: -lengths.float()                  # noqa: E731  (toy host reward: shorter answers are better)
    out = trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), 1, reward, samples=3, baseline="greedy",
                                     rollout=rollout, max_answer_len=MAXLEN, seed=4, no_repeat_ngram_size=2)
    torch.cuda.synchronize()
    assert all(math.isfinite(v) for v in out), out
    assert len(calls) == (1 if rollout == "fused" else 2)
    for call in calls:                                                 # samples and baseline decode under one rule
        assert call["no_repeat_ngram_size"] == 2 and call["repetition_penalty"] == 1.0 and call["repeat_scope"] == "answer"
        res = call["result"]
        for part in (res, res.greedy) if res.greedy is not None else (res,):
            for g, j, ans in all_answers(part):
                assert not CR.repeats_ngram(ans, 2), (rollout, g, j, ans)
