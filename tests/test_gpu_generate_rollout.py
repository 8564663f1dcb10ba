"""One rollout for self-critical training on the GPU: generate_answers(samples=N, greedy=True) -- the samples and the greedy
baseline in one prefill and one walk over the decode steps -- against the CPU oracle with the gates of
tests/test_gpu_generate.py, against the two separate calls it replaces, at the decode kernel's slot bound, against
sequence_log_likelihood on the full config, and through trainer.self_critical_step(rollout="fused").  The model and dialog
builders are those of tests/test_gpu_generate.py, the sampled-answer helpers those of tests/test_gpu_generate_sample.py."""
import math

import pytest
import torch

from tests.test_gpu_generate import (SEP, answers_of, banned_row, completed, full, gen_kwargs, make_dialogs, oracle_steps,  # noqa: F401
                                     tiny)
from tests.test_gpu_generate_sample import flat, undecided_in_oracle

pytestmark = pytest.mark.gpu
T_TINY, G_TINY, MAXLEN, SAMPLES, SEED = 64, 6, 8, 4, 3
MARGIN = 0.05


def tiny_dialogs():
    return make_dialogs(G_TINY, T_TINY, 1000, 37, 192, seed=1, cmin=8, cmax=40)


def generate(model, d, c, **kw):
    kw.setdefault("max_answer_len", MAXLEN)
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, **gen_kwargs(d), **kw)
    torch.cuda.synchronize()
    return res


def flat_greedy(res):
    """[(g, 0, answer tokens, n)] of a beams = 1 shaped result with the invariants of every greedy answer."""
    out = []
    assert res.step_logq is None and res.greedy is None and res.lengths.shape[1] == 1
    for g in range(res.lengths.shape[0]):
        ans, n = answers_of(res, g, 0)
        assert n >= 2 and res.tokens[g, 0, n - 1] == SEP and not set(ans) & {0, 101, 103, SEP}
        assert (res.tokens[g, 0, n:] == 0).all() and (res.step_logp[g, 0, n:] == 0).all()
        out.append((g, 0, ans, n))
    return out


def limit_of(c, g):
    return min(MAXLEN, (T_TINY - int(c[g])) // 2 - 1)


@pytest.fixture(scope="module")
def rollout(tiny):
    """The fused call and the two calls it replaces (same seed), once for the module."""
    model, _, _ = tiny
    d, c, utts = tiny_dialogs()
    fused = generate(model, d, c, samples=SAMPLES, greedy=True, seed=SEED)
    samples = generate(model, d, c, samples=SAMPLES, seed=SEED)
    greedy = generate(model, d, c, beams=1)
    return d, c, utts, fused, samples, greedy


def test_fused_call_against_the_oracle(tiny, rollout):
    """step_logp within 1e-2 + 1e-2 |want| of the teacher-forced oracle, logp within 1e-2 n + 1e-2 |sum|, for the samples and the
    greedy slot; on every step whose oracle top-2 margin (after the step rules) exceeds 0.05 the greedy token is the oracle's
    argmax, and such steps are at least 80 % of the greedy steps (the gates of tests/test_gpu_generate.py)."""
    _, ocfg, sd = tiny
    d, c, utts, res, _, _ = rollout
    assert res.tokens.shape == (G_TINY, SAMPLES, MAXLEN + 1) and res.greedy.tokens.shape == (G_TINY, 1, MAXLEN + 1)
    assert res.step_logq.shape == res.tokens.shape and res.greedy.scores.shape == res.greedy.logp.shape == (G_TINY, 1)
    rows = [(res, r) for r in flat(res)] + [(res.greedy, r) for r in flat_greedy(res.greedy)]
    steps = oracle_steps(ocfg, sd, d, [r[0] for _, r in rows], utts, [r[2] for _, r in rows], T_TINY)
    clear = total = 0
    for (out, (g, j, ans, n)), lp in zip(rows, steps):
        toks = ans + [SEP]
        want = torch.stack([lp[k, t] for k, t in enumerate(toks)])
        got = out.step_logp[g, j, :n].double().cpu()
        assert ((got - want).abs() <= 1e-2 + 1e-2 * want.abs()).all(), (g, j, got, want)
        assert abs(float(out.logp[g, j]) - float(want.sum())) <= 1e-2 * n + 1e-2 * abs(float(want.sum()))
        assert abs(float(out.scores[g, j]) - float(out.logp[g, j])) == 0.0                  # length_penalty = 0
        if out is res.greedy:
            for k, t in enumerate(toks):
                top2 = torch.topk(banned_row(lp[k], k, limit_of(c, g)), 2).values
                total += 1
                if float(top2[0] - top2[1]) > MARGIN:
                    clear += 1
                    assert int(torch.argmax(banned_row(lp[k], k, limit_of(c, g)))) == t, (g, k)
        else:
            assert (out.step_logq[g, j, :n] >= out.step_logp[g, j, :n] - 1e-5).all()
    print(f"\ngreedy slot: {clear} of {total} steps with an oracle top-2 margin above {MARGIN}")
    assert clear >= 0.8 * total


def test_fused_against_the_separate_calls(tiny, rollout):
    """Per (dialog, slot) the tokens may first differ from the separate call's only at a step the oracle cannot separate (greedy:
    top-2 margin <= 0.05; a sample: undecided_in_oracle); identical answers agree in step_logp to 1e-3 |value| + 1e-5."""
    _, ocfg, sd = tiny
    d, c, utts, res, samples, greedy = rollout
    flat(res), flat(samples), flat_greedy(res.greedy), flat_greedy(greedy)
    same = differ = 0
    pairs = [(res.greedy, greedy, g, 0) for g in range(G_TINY)] + [(res, samples, g, j) for g in range(G_TINY) for j in range(SAMPLES)]
    for a, b, g, j in pairs:
        x, y = a.tokens[g, j].tolist(), b.tokens[g, j].tolist()
        if x == y:
            same += 1
            assert int(a.lengths[g, j]) == int(b.lengths[g, j])
            u, v = a.step_logp[g, j], b.step_logp[g, j]
            assert ((u - v).abs() <= 1e-3 * v.abs() + 1e-5).all(), (g, j, u, v)
            if a is res:
                u, v = a.step_logq[g, j], b.step_logq[g, j]
                assert ((u - v).abs() <= 1e-3 * v.abs() + 1e-5).all(), (g, j, u, v)
            continue
        differ += 1
        k = next(i for i, (p, q) in enumerate(zip(x, y)) if p != q)
        if a is res:
            assert undecided_in_oracle(ocfg, sd, d, utts, c, g, x[:k], k, SEED, g * SAMPLES + j), (g, j, k)
        else:
            lp = oracle_steps(ocfg, sd, d, [g], utts, [x[:k]], T_TINY)[0][k]
            top2 = torch.topk(banned_row(lp, k, limit_of(c, g)), 2).values
            assert float(top2[0] - top2[1]) <= MARGIN, (g, k, top2)
    print(f"\nfused against separate calls: {same} of {len(pairs)} answers identical, {differ} differ at an undecided step")
    assert same > 0                                                    # the step_logp comparison above is not vacuous


def test_which_draw_kernel_runs(tiny, monkeypatch):
    """Per-draw parameters or greedy=True draw with unimm_lm_sample_rows, a call with neither with unimm_lm_sample as before; a
    draw with top_k = 1 has log q = 0 on every token, the other draws of the launch do not."""
    from unimm_amd import generation as GN
    model, _, _ = tiny
    d, c, _ = tiny_dialogs()
    counts = dict(lm_sample=0, lm_sample_rows=0)
    for name in counts:
        def counted(*a, _f=getattr(GN.L, name), _n=name, **kw):
            counts[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(GN.L, name, counted)
    plain = generate(model, d, c, samples=SAMPLES, seed=SEED, top_k=20, temperature=0.8)
    assert counts["lm_sample"] >= 2 and counts["lm_sample_rows"] == 0 and plain.greedy is None
    counts.update(lm_sample=0)
    per = generate(model, d, c, samples=SAMPLES, seed=SEED, top_k=[20, 1, 0, 20], temperature=[0.8, 0.7, 1.0, 2.0], top_p=0.9)
    assert counts["lm_sample"] == 0 and counts["lm_sample_rows"] >= 2 and per.greedy is None
    flat(per)
    assert (per.step_logq[:, 1] == 0).all() and (per.step_logq[:, 0] != 0).any() and (per.step_logq[:, 2] != 0).any()
    counts.update(lm_sample_rows=0)
    both = generate(model, d, c, samples=SAMPLES, seed=SEED, greedy=True)
    assert counts["lm_sample"] == 0 and counts["lm_sample_rows"] >= 2 and both.greedy is not None


def test_slot_bounds(tiny):
    """15 samples and the greedy slot are 16 slots, 32 query rows per dialog: unimm_attn_decode's bound.  16 samples with the
    greedy slot are refused."""
    model, _, _ = tiny
    d, c, _ = make_dialogs(2, T_TINY, 1000, 37, 192, seed=1, cmin=8, cmax=40)
    res = generate(model, d, c, samples=15, greedy=True, seed=SEED)
    assert res.tokens.shape == (2, 15, MAXLEN + 1) and res.greedy.tokens.shape == (2, 1, MAXLEN + 1)
    assert len(flat(res)) == 30 and len(flat_greedy(res.greedy)) == 2
    assert torch.isfinite(res.logp).all() and torch.isfinite(res.greedy.logp).all()
    for g in range(2):
        assert len({tuple(res.tokens[g, j].tolist()) for j in range(15)}) > 1
    with pytest.raises(ValueError, match="32 query rows"):
        generate(model, d, c, samples=16, greedy=True, seed=SEED)
    with pytest.raises(ValueError, match="beams=1"):
        generate(model, d, c, greedy=True)


def test_full_config_logp_equals_sequence_log_likelihood(full):
    """G = 6, three samples and the greedy slot, max_answer_len = 6: every logp equals sequence_log_likelihood of the completed
    sequence within 2e-3 of the largest |score| (the gate of tests/test_gpu_generate_sample.py for the same identity)."""
    model, _, _ = full
    T, G, N = 256, 6, 3
    d, c, utts = make_dialogs(G, T, 30522, 37, 2048, seed=77, cmin=10, cmax=200)
    res = generate(model, d, c, samples=N, greedy=True, max_answer_len=6, top_p=0.9, temperature=0.8, seed=2)
    rows = [(res, r) for r in flat(res)] + [(res.greedy, r) for r in flat_greedy(res.greedy)]
    assert len(rows) == G * (N + 1)
    gs = [r[0] for _, r in rows]
    seq, _ = completed([utts[g] for g in gs], [r[2] for _, r in rows], T)
    dev = "cuda"
    want, _ = model.sequence_log_likelihood(seq["tokens"].to(dev), d["image_feat"][gs].to(dev), d["image_loc"][gs].to(dev),
                                            seq["labels"].to(dev), token_type_ids=seq["segments"].to(dev),
                                            position_ids=seq["positions"].to(dev), attention_mask=seq["txt_attention_mask"].to(dev),
                                            co_attention_mask=seq["co_attention_mask"].to(dev),
                                            image_attention_mask=d["image_attention_mask"][gs].to(dev))
    got = torch.stack([out.logp[g, j] for out, (g, j, _, _) in rows]).cpu()
    want = want.cpu()
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"\nG = {G}, {N} samples + greedy: logp {float(got.min()):.3f} .. {float(got.max()):.3f}, "
          f"|rollout - sequence_log_likelihood| {err:.3e} ({err / scale:.2e} of scale)")
    assert err <= 2e-3 * scale


@pytest.mark.parametrize("shared_context", [False, True])
def test_self_critical_step_fused_rollout(shared_context):
    from tests.test_gpu_policy_model import _encoder
    from unimm_amd import trainer
    from unimm_amd.policy import PolicyObjective
    enc, opt, sch = _encoder()
    d, c, _ = make_dialogs(4, T_TINY, 1000, 37, 192, seed=8, cmin=8, cmax=40)
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"])
    eng = enc.bert_pretrained.engine
    eng.ensure(torch.device("cuda", 0))
    p0 = eng.arena.flat.clone()
    calls, real = [], enc.generate_answers

    def counted(*a, **kw):
        calls.append(kw)
        calls[-1]["result"] = real(*a, **kw)
        return calls[-1]["result"]

    enc.generate_answers = counted
    reward = lambda tokens, lengths: -lengths.float()                  # noqa: E731  (toy host reward: shorter answers are better)
    with pytest.raises(ValueError, match="baseline='greedy'"):
        trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), 1, reward, samples=3, baseline="mean",
                                   rollout="fused", max_answer_len=MAXLEN, seed=4)
    assert not calls and torch.equal(p0, eng.arena.flat)
    out = trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), 1, reward, samples=3, baseline="greedy",
                                     rollout="fused", objective=PolicyObjective(), max_answer_len=MAXLEN, seed=4,
                                     shared_context=shared_context)
    torch.cuda.synchronize()
    loss, mean_reward, mean_baseline, mean_entropy = out
    print(f"\nself_critical_step(fused, shared_context={shared_context}): loss {loss:.4f} reward {mean_reward:.3f} baseline "
          f"{mean_baseline:.3f} entropy {mean_entropy:.4f}")
    assert len(calls) == 1 and calls[0]["samples"] == 3 and calls[0]["greedy"] is True and "beams" not in calls[0]
    res = calls[0]["result"]
    assert res.tokens.shape[:2] == (4, 3) and res.greedy.tokens.shape[:2] == (4, 1)
    # the baseline is the greedy slot's reward: mean over the samples of (the dialog's greedy reward)
    assert abs(mean_baseline - float((-res.greedy.lengths.float()).mean())) <= 1e-5
    assert all(math.isfinite(v) for v in out)
    assert mean_entropy > 0 and -MAXLEN - 1 <= mean_reward <= -1
    assert enc.training
    assert not torch.equal(p0, eng.arena.flat), "the optimizer stepped"
    assert torch.isfinite(eng.arena.flat).all()
