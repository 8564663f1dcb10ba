"""Speculative sampling on the GPU: `generate_answers(draft=..., draft_accept="rejection", samples=N)` on the tiny model of
tests/test_gpu_speculative.py (drafts A, a frozen copy, and B, another initialisation with the model's decoder bias) -- against the
greedy calls where every row keeps one id, against the float64 oracle teacher-forced, the invariants of every sampled answer, the
acceptance record, repeatability, the greedy slot, no side effects, the plain calls' launches, and through
trainer.self_critical_step(draft=...)."""
import numpy as np
import pytest
import torch

from tests import test_gpu_generate as TG
from tests import test_gpu_generate_edges as TE
from tests.test_gpu_generate_sample import flat
from tests.test_gpu_speculative import w  # noqa: F401  (the module-scoped models, dialogs and oracle cache)

pytestmark = pytest.mark.gpu
SEP = 102
T, MAXLEN, G, N = 96, 6, 3, 3


def call(w, name, gamma, n=N, **kw):  # noqa: F811
    d = {k: v[:G] for k, v in w["d"].items()}
    kw.setdefault("samples", n)
    kw.setdefault("max_answer_len", MAXLEN)
    res = w["model"].generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], w["c"][:G], draft=w["drafts"][name],
                                      draft_len=gamma, draft_accept=kw.pop("draft_accept", "rejection"), **TG.gen_kwargs(d), **kw)
    torch.cuda.synchronize()
    return res


def counters_add_up(res, gamma):
    sp = res.speculation
    Gn, Nn = res.lengths.shape
    assert sp.drafted.shape == sp.accepted.shape == (Gn, Nn) and sp.per_round.shape == (sp.rounds, Gn, Nn)
    live = (sp.per_round >= 0).sum(0)
    assert torch.equal(sp.drafted, gamma * live) and torch.equal(sp.accepted, sp.per_round.clamp_min(0).sum(0))
    own = res.lengths - 1 - sp.accepted                                # tokens that were residual or bonus draws
    assert ((own == live) | (own == live - 1)).all() and (sp.accepted <= sp.drafted).all()


@pytest.mark.parametrize("gamma", [1, 3])
def test_one_greedy_sample_is_the_greedy_calls(w, gamma):  # noqa: F811
    d = {k: v[:G] for k, v in w["d"].items()}
    plain = w["model"].generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], w["c"][:G], beams=1, max_answer_len=MAXLEN,
                                        **TG.gen_kwargs(d))
    match = call(w, "B", gamma, samples=0, beams=1, draft_accept="match")
    one = call(w, "B", gamma, n=1, top_k=1, temperature=0.7, seed=9)
    for ref in (plain, match):
        assert torch.equal(one.tokens, ref.tokens) and torch.equal(one.lengths, ref.lengths)
        assert (one.step_logp - ref.step_logp).abs().max().item() <= 1e-5
    assert (one.step_logq == 0).all()
    assert torch.equal(one.speculation.accepted[:, 0], match.speculation.accepted) and one.speculation.rounds == match.speculation.rounds
    counters_add_up(one, gamma)


@pytest.mark.parametrize("gamma", [1, 3])
def test_a_frozen_copy_is_always_accepted_and_the_oracle_agrees(w, gamma):  # noqa: F811
    """Draft A computes the model's logits (the same kernels on the same rows up to the batch shape of its decode steps), so
    log P~ - log Q~ is ~0 and a draft is rejected only where log u > -|rounding|: every draft inside an answer is accepted.  The
    invariants of `flat`, step_logp / logp teacher-forced against the float64 oracle at the gates of
    tests/test_gpu_generate_sample.py, step_logq >= step_logp - 1e-5."""
    res = call(w, "A", gamma, temperature=1.0, seed=3)
    rows = flat(res)
    counters_add_up(res, gamma)
    sp = res.speculation
    # every draft of a round was accepted, up to the [SEP] that ended the answer: the round's count is min(gamma, tokens left)
    n = torch.ones_like(res.lengths)
    for r in range(sp.rounds):
        a = sp.per_round[r]
        livem = a >= 0
        assert torch.equal(a[livem], torch.minimum(torch.full_like(a, gamma), res.lengths - n)[livem]), (r, a, res.lengths, n)
        n = n + torch.where(livem, torch.minimum(a + 1, res.lengths - n), 0)
    assert torch.equal(n, res.lengths)
    d = {k: v[:G] for k, v in w["d"].items()}
    steps = TG.oracle_steps(w["ocfg"], w["sd"], d, [g for g, _, _, _ in rows], w["utts"][:G], [a for _, _, a, _ in rows], T)
    for (g, j, ans, n_), lp in zip(rows, steps):
        toks = ans + [SEP]
        want = torch.stack([lp[k, t] for k, t in enumerate(toks)])
        got = res.step_logp[g, j, :n_].double().cpu()
        assert ((got - want).abs() <= 1e-2 + 1e-2 * want.abs()).all(), (g, j, got, want)
        assert abs(float(res.logp[g, j]) - float(want.sum())) <= 1e-2 * n_ + 1e-2 * abs(float(want.sum()))
        assert float(res.scores[g, j]) == float(res.logp[g, j])
        assert (res.step_logq[g, j, :n_] >= res.step_logp[g, j, :n_] - 1e-5).all()
        assert len(ans) <= w["limits"][g]


def test_another_initialisation_as_draft(w):  # noqa: F811
    res = call(w, "B", 3, seed=5, top_k=[0, 20, 0], top_p=[1.0, 0.9, 0.8], temperature=[1.0, 0.8, 1.3], greedy=True)
    flat(res)
    counters_add_up(res, 3)
    sp = res.speculation
    rate = int(sp.accepted.sum()) / int(sp.drafted.sum())
    print(f"\ndraft B, draft_len 3: accepted {int(sp.accepted.sum())} of {int(sp.drafted.sum())} drafts in {sp.rounds} rounds")
    assert 0.0 < rate < 1.0
    again = call(w, "B", 3, seed=5, top_k=[0, 20, 0], top_p=[1.0, 0.9, 0.8], temperature=[1.0, 0.8, 1.3], greedy=True)
    for f in ("tokens", "lengths", "logp", "step_logp", "step_logq"):
        assert torch.equal(getattr(res, f), getattr(again, f)), f
    assert torch.equal(res.greedy.tokens, again.greedy.tokens) and torch.equal(sp.per_round, again.speculation.per_round)
    other = call(w, "B", 3, seed=6, top_k=[0, 20, 0], top_p=[1.0, 0.9, 0.8], temperature=[1.0, 0.8, 1.3], greedy=True)
    assert not torch.equal(other.tokens, res.tokens)
    d = {k: v[:G] for k, v in w["d"].items()}
    plain = w["model"].generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], w["c"][:G], beams=1, max_answer_len=MAXLEN,
                                        **TG.gen_kwargs(d))
    gr = res.greedy
    assert gr.tokens.shape == plain.tokens.shape and gr.step_logq is None
    assert torch.equal(gr.tokens, plain.tokens) and torch.equal(gr.lengths, plain.lengths)
    assert (gr.step_logp - plain.step_logp).abs().max().item() <= 1e-5 and (gr.logp - plain.logp).abs().max().item() <= 1e-4
    assert torch.equal(other.greedy.tokens, plain.tokens)


def test_sep_is_forced_at_mixed_limits(w):  # noqa: F811
    model = w["model"]
    d, c, _ = TE.exact_dialogs(TE.LIMIT_CONTEXTS[3], seed=53)
    lim = np.minimum(TE.MAXLEN, (TE.T - c) // 2 - 1)
    assert len(set(lim.tolist())) > 1
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, samples=2, max_answer_len=TE.MAXLEN,
                                 min_answer_len=1, draft=w["drafts"]["B"], draft_len=3, draft_accept="rejection", seed=2,
                                 temperature=3.0, **TG.gen_kwargs(d))
    torch.cuda.synchronize()
    hit = 0
    for g, j, ans, n in flat(res):
        assert 1 <= len(ans) <= lim[g] or lim[g] == 0
        if len(ans) == lim[g]:                                         # the answer ran into its limit: [SEP] was the one id left
            hit += 1
            assert float(res.step_logq[g, j, n - 1]) == 0.0
    assert hit >= 1


def test_no_side_effects_and_plain_calls_launch_what_they_launched(w, monkeypatch):  # noqa: F811
    from unimm_amd import lib as L
    model, draft = w["model"], w["drafts"]["B"]
    d = {k: v[:G] for k, v in w["d"].items()}
    seq, _ = TG.completed(w["utts"][:G], [[200, 300]] * G, T)
    sargs = (seq["tokens"].cuda(), d["image_feat"].cuda(), d["image_loc"].cuda(), seq["labels"].cuda())
    skw = dict(token_type_ids=seq["segments"].cuda(), position_ids=seq["positions"].cuda(),
               attention_mask=seq["txt_attention_mask"].cuda(), co_attention_mask=seq["co_attention_mask"].cuda(),
               image_attention_mask=d["image_attention_mask"].cuda())
    calls = []
    real = L._call
    monkeypatch.setattr(L, "_call", lambda name, *a: (calls.append(name), real(name, *a))[1])

    def plain():
        calls.clear()
        L.prof_enable(True)
        try:
            res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], w["c"][:G], samples=N, seed=4, top_p=0.9,
                                         max_answer_len=MAXLEN, **TG.gen_kwargs(d))
            torch.cuda.synchronize()
            prof = {k: v[2] for k, v in L.prof_collect().items()}
        finally:
            L.prof_enable(False)
        return res, prof, [n for n in calls if not n.startswith("unimm_prof")]

    first = plain()
    before = [m.sequence_log_likelihood(*sargs, **skw)[0] for m in (model, draft)]
    counters = [m._engine.step for m in (model, draft)]
    calls.clear()
    call(w, "B", 3, seed=4, top_p=0.9)
    assert "unimm_lm_spec_verify" in calls and "unimm_attn_verify" in calls
    after = [m.sequence_log_likelihood(*sargs, **skw)[0] for m in (model, draft)]
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    assert model.training is False and draft.training is False
    assert counters == [m._engine.step for m in (model, draft)]
    second = plain()
    assert first[1] == second[1] and sum(first[1].values()) > 0 and first[2] == second[2]
    assert not {"unimm_lm_spec_verify", "unimm_attn_verify", "unimm_kv_cache_append"} & set(second[2])
    for f in ("tokens", "lengths", "logp", "step_logp", "step_logq"):
        assert torch.equal(getattr(first[0], f), getattr(second[0], f)), f


@pytest.mark.parametrize("rollout", ["separate", "fused"])
def test_self_critical_step_with_a_draft(rollout):
    from tests.test_gpu_policy_model import _encoder
    from unimm_amd import trainer
    from unimm_amd.policy import frozen_reference
    enc, opt, sch = _encoder()
    draft = frozen_reference(enc)
    d, c, _ = TG.make_dialogs(3, 64, 1000, 37, 192, seed=8, cmin=8, cmax=40)
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"])
    calls, real = [], enc.generate_answers

    def counted(*a, **kw):
        calls.append(kw)
        calls[-1]["result"] = real(*a, **kw)
        return calls[-1]["result"]

    enc.generate_answers = counted
    out = trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), 1, lambda tokens, lengths: -lengths.float(),
                                     samples=3, rollout=rollout, max_answer_len=MAXLEN, seed=4, draft=draft, draft_len=2)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in out), out
    assert calls[0]["draft_accept"] == "rejection" and calls[0]["draft"] is draft and calls[0]["draft_len"] == 2
    assert calls[0]["result"].speculation is not None and calls[0]["result"].step_logq is not None
    if rollout == "separate":
        assert len(calls) == 2 and calls[1]["draft"] is draft and "draft_accept" not in calls[1]
        assert calls[1]["result"].speculation is not None
    else:
        assert len(calls) == 1 and calls[0]["greedy"] is True and calls[0]["result"].greedy.speculation is not None
