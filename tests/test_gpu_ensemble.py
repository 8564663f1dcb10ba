"""Ensemble and contrastive answer generation on the GPU: `generate_answers(ensemble=...)` on the tiny model of
tests/test_gpu_generate.py, G = 4 dialogs, answers of up to 8 tokens, with two partners -- A a frozen copy of the model, B another
initialisation with another depth -- against the plain call (bit for bit where the mixture IS the model) and against the float64
oracle of both models teacher-forced on the returned answers."""
import json
import os

import numpy as np
import pytest
import torch

from tests import mix_ref as MR
from tests import test_gpu_generate as TG
from tests import test_gpu_generate_edges as TE

pytestmark = pytest.mark.gpu
SEP = 102
T, MAXLEN, G = 64, 8, 4
ROOT = TG.ROOT
FIELDS = ("tokens", "lengths", "scores", "logp", "step_logp")
KERNEL_BUDGET = 4 * MR.PROB_BUDGET              # the device budget of a PROB row (tests/test_gpu_mix_edges.py); measured here: 9.5e-07


@pytest.fixture(scope="module")
def w():
    from oracle import vilbert_ref as R
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    from unimm_amd.policy import frozen_reference
    cfgd = json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json")))
    ocfg = R.make_config(cfgd)
    sd = R.init_state_dict(ocfg, seed=11)
    sd["cls.predictions.bias"] = torch.randn(sd["cls.predictions.bias"].shape, generator=torch.Generator().manual_seed(5)) * 3.0
    model = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd))
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    cfgb = dict(cfgd, num_hidden_layers=3, t_biattention_id=[1, 2])          # one text layer fewer, its own schedule
    ocfgb = R.make_config(cfgb)
    sdb = R.init_state_dict(ocfgb, seed=12)
    sdb["cls.predictions.bias"] = torch.randn(sdb["cls.predictions.bias"].shape, generator=torch.Generator().manual_seed(6)) * 3.0
    other = BertForMultiModalPreTraining(BertConfig.from_dict(cfgb))
    other.load_state_dict(sdb, strict=True)
    d, c, utts = TG.make_dialogs(G, T, 1000, 37, 192, seed=31, cmin=8, cmax=40)
    out = dict(model=model, A=frozen_reference(model), A2=frozen_reference(model), B=other.cuda().eval(), ocfg=ocfg, sd=sd,
               ocfgb=ocfgb, sdb=sdb, d=d, c=c, utts=utts, limits=np.minimum(MAXLEN, (T - c) // 2 - 1), plain={})
    return out


def call(w, d=None, c=None, **kw):
    d, c = w["d"] if d is None else d, w["c"] if c is None else c
    res = w["model"].generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, max_answer_len=MAXLEN,
                                      **{**TG.gen_kwargs(d), **kw})
    torch.cuda.synchronize()
    return res


FORMS = dict(beams1=dict(beams=1), beams3=dict(beams=3), samples4=dict(samples=4, seed=7, temperature=0.9, top_p=0.95),
             greedy=dict(samples=3, seed=8, greedy=True))


def plain(w, form):
    if form not in w["plain"]:
        w["plain"][form] = call(w, **FORMS[form])
    return w["plain"][form]


def same_bits(a, b, sampled):
    for f in FIELDS + (("step_logq",) if sampled else ()):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert (a.greedy is None) == (b.greedy is None)
    if a.greedy is not None:
        same_bits(a.greedy, b.greedy, False)


def record_calls(mp):
    """-> the list that fills with the C entry points called by name, in order: the main library's and the extension library's"""
    from unimm_amd import lib as L
    from unimm_amd import mix as MX
    calls = []
    for mod in (L, MX):
        mp.setattr(mod, "_call", lambda name, *a, real=mod._call: (calls.append(name), real(name, *a))[1])
    return calls


@pytest.mark.parametrize("form", list(FORMS))
def test_two_copies_in_logit_halves_are_the_plain_call(w, form):
    """0.5 x + 0.5 x is x in fp32, so every selection launch reads the bits it reads in the plain call"""
    got = call(w, ensemble=[w["A"]], ensemble_weights=[0.5, 0.5], ensemble_mode="logit", **FORMS[form])
    same_bits(got, plain(w, form), "samples" in FORMS[form])
    assert int(got.lengths.min()) >= 2


def test_two_copies_in_prob_mode(w):
    got, ref = call(w, ensemble=[w["A"]], ensemble_weights=[0.3, 0.7], ensemble_mode="prob", beams=1), plain(w, "beams1")
    assert torch.equal(got.tokens, ref.tokens) and torch.equal(got.lengths, ref.lengths)
    err = float((got.step_logp - ref.step_logp).abs().max())
    print(f"\nPROB (0.3, 0.7) of two copies: max |step_logp - plain| = {err:.3e} (budget {KERNEL_BUDGET:.3e})")
    assert err <= KERNEL_BUDGET


def test_a_partner_of_weight_zero_changes_nothing(w, monkeypatch):
    """partner B (another initialisation and depth), LOGIT (1, 0): 1 x + 0 y is x -- and the partner did run"""
    calls = record_calls(monkeypatch)
    for form in ("beams1", "beams3"):
        ref = plain(w, form)
        calls.clear()
        got = call(w, ensemble=[w["B"]], ensemble_weights=[1.0, 0.0], ensemble_mode="logit", **FORMS[form])
        same_bits(got, ref, False)
        steps = calls.count("unimm_lm_mix")
        assert steps == calls.count("unimm_lm_topk") >= 2 and calls.count("unimm_attn_decode") == (4 + 3) * (steps - 1)


def oracle_mixture(w, res, members, weights, beams):
    """Teacher-force the float64 oracle of every member on the returned answers -> per (g, b): (answer, n, log of the weighted sum
    of the members' step distributions [steps, V])"""
    idx, answers, rows = [], [], []
    for g in range(G):
        for b in range(beams):
            ans, n = TG.answers_of(res, g, b)
            assert n >= 2 and res.tokens[g, b, n - 1] == SEP and not set(ans) & {0, 101, 103, SEP} and len(ans) <= w["limits"][g]
            idx.append(g)
            answers.append(ans)
            rows.append((g, b, n))
    steps = [TG.oracle_steps(ocfg, sd, w["d"], idx, w["utts"], answers, T) for ocfg, sd in members]
    out = []
    for i, (g, b, n) in enumerate(rows):
        mix = torch.logsumexp(torch.stack([s[i] + float(np.log(wt)) for s, wt in zip(steps, weights)]), 0)
        out.append((g, b, n, answers[i], mix))
    return out


def check_against_oracle(w, res, members, weights, beams):
    clear = total = 0
    for g, b, n, ans, lp in oracle_mixture(w, res, members, weights, beams):
        toks = ans + [SEP]
        want = torch.stack([lp[k, t] for k, t in enumerate(toks)])
        got = res.step_logp[g, b, :n].double().cpu()
        assert ((got - want).abs() <= 1e-2 + 1e-2 * want.abs()).all(), (g, b, got, want)        # test_gpu_generate.py's gate
        assert abs(float(res.logp[g, b]) - float(want.sum())) <= 1e-2 * n + 1e-2 * abs(float(want.sum()))
        if beams == 1:
            for k, t in enumerate(toks):
                row = TG.banned_row(lp[k], k, int(w["limits"][g]))
                top2 = torch.topk(row, 2).values
                total += 1
                if float(top2[0] - top2[1]) > 0.05:
                    clear += 1
                    assert int(torch.argmax(row)) == t, (g, k)
    return clear, total


@pytest.mark.parametrize("beams", [1, 3])
def test_prob_mixture_against_the_oracle_of_both_models(w, beams):
    res = call(w, ensemble=[w["B"]], ensemble_weights=[0.6, 0.4], beams=beams)
    clear, total = check_against_oracle(w, res, [(w["ocfg"], w["sd"]), (w["ocfgb"], w["sdb"])], [0.6, 0.4], beams)
    if beams == 1:
        print(f"\nPROB (0.6, 0.4): {clear} of {total} greedy steps with an oracle mixture margin above 0.05")
        assert clear >= 0.75 * total
        assert not torch.equal(res.tokens, plain(w, "beams1").tokens)          # the partner moved the answers


def test_three_members_with_uneven_weights(w):
    res = call(w, ensemble=[w["A"], w["B"]], ensemble_weights=[0.5, 0.2, 0.3], beams=1)
    check_against_oracle(w, res, [(w["ocfg"], w["sd"]), (w["ocfgb"], w["sdb"])], [0.7, 0.3], 1)   # A is the model again


def test_a_cut_just_below_one_leaves_the_models_greedy_answer(w):
    """plausibility = 0.999999: only the model's own best id (and [SEP]) survive every step, whatever the contrast says"""
    res = call(w, ensemble=[w["B"]], ensemble_weights=[1.5, -0.5], ensemble_mode="logit", plausibility=0.999999, beams=1)
    ref = plain(w, "beams1")
    assert torch.equal(res.tokens, ref.tokens) and torch.equal(res.lengths, ref.lengths)
    assert torch.isfinite(res.logp).all() and (res.step_logp <= 0).all()


def test_mixed_limits_and_min_answer_len(w):
    cs = [56, 54, 30, 12]
    d, c, utts = TE.exact_dialogs(cs, seed=53)
    lim = np.minimum(MAXLEN, (T - c) // 2 - 1)
    assert sorted(set(lim.tolist())) == [3, 4, 8]
    for beams in (1, 3):
        ref = call(w, d, c, beams=beams, min_answer_len=3)
        same_bits(call(w, d, c, beams=beams, min_answer_len=3, ensemble=[w["A"]], ensemble_weights=[0.5, 0.5], ensemble_mode="logit"),
                  ref, False)
        res = call(w, d, c, beams=beams, min_answer_len=3, ensemble=[w["A"], w["B"]], ensemble_mode="prob", plausibility=0.05)
        for g in range(G):
            for b in range(beams):
                n = int(res.lengths[g, b])
                if n == 0:
                    continue
                assert 4 <= n <= lim[g] + 1 and res.tokens[g, b, n - 1] == SEP and SEP not in res.tokens[g, b, :n - 1].tolist()
                assert torch.isfinite(res.step_logp[g, b, :n]).all()
        assert (res.lengths[:, 0] > 0).all()


def test_a_partner_on_a_text_stream_of_its_own(w):
    """A partner whose engine keeps a high-priority text stream (`text_priority`): its prefill, decode steps and cache updates
    run there, and `Engine._on_text_stream` brackets each with a wait in both directions, so the mix -- on the model's stream --
    reads finished rows.  Two copies in LOGIT halves then still give the plain call's bits, for beams and for samples, three
    times over (a missing wait shows as other bits, not on every run)."""
    eng = w["A2"]._engine
    assert eng.text_priority is False
    eng.text_priority = True
    try:
        for form in ("beams3", "samples4"):
            for _ in range(3):
                got = call(w, ensemble=[w["A2"]], ensemble_weights=[0.5, 0.5], ensemble_mode="logit", **FORMS[form])
                same_bits(got, plain(w, form), "samples" in FORMS[form])
        assert eng._dual() and eng._tstream is not None       # the partner did run on a stream of its own
    finally:
        eng.text_priority = False


def test_no_side_effects(w):
    members = (w["model"], w["A"], w["B"])
    before = [[p.detach().clone() for p in m.parameters()] for m in members]
    ref = plain(w, "beams1")
    call(w, ensemble=[w["A"], w["B"]], ensemble_weights=[0.5, 0.25, 0.25], beams=3)
    call(w, ensemble=[w["B"]], ensemble_weights=[1.5, -0.5], ensemble_mode="logit", plausibility=0.1, samples=2, seed=3)
    again = call(w, beams=1)
    same_bits(again, ref, False)
    for m, saved in zip(members, before):
        for p, q in zip(m.parameters(), saved):
            assert torch.equal(p, q)
        assert m.training is False


def recorded(w, monkeypatch, **kw):
    """(result, the launch profiler's GEMM counts, the C entry points in call order) of one call"""
    from unimm_amd import lib as L
    with monkeypatch.context() as mp:
        calls = record_calls(mp)
        L.prof_enable(True)
        try:
            res = call(w, **kw)
            prof = {k: v[2] for k, v in L.prof_collect().items()}
        finally:
            L.prof_enable(False)
    return res, prof, [n for n in calls if not n.startswith("unimm_prof")]


def test_without_an_ensemble_the_call_is_launch_for_launch_what_it_was(w, monkeypatch):
    """What this can show inside one build (the strength of the speculative test it follows, not a comparison with an older
    build): a plain call does not call unimm_lm_mix, the new keywords spelled out at their defaults change neither the launch
    profiler's record nor the C entry points called, and the bits are the plain call's."""
    a = recorded(w, monkeypatch, beams=3)
    b = recorded(w, monkeypatch, beams=3, ensemble=None, ensemble_weights=None, ensemble_mode="prob", plausibility=0.0)
    assert a[1] == b[1] and sum(a[1].values()) > 0 and a[2] == b[2]
    assert "unimm_lm_mix" not in a[2] and "unimm_attn_decode" in a[2] and a[2][-1] == "unimm_lm_topk"
    same_bits(a[0], b[0], False)
    same_bits(a[0], plain(w, "beams3"), False)


def split(calls, at):
    out, cur = [], []
    for n in calls:
        if n == at:
            out.append(cur)
            cur = []
        else:
            cur.append(n)
    return out


def test_launch_order_of_an_ensemble_step(w, monkeypatch):
    """A step of an ensemble of K members of one architecture: K cache updates, K times the side's launches, ONE unimm_lm_mix,
    then the selection launch."""
    K = 3
    one = split(recorded(w, monkeypatch, beams=3)[2], "unimm_lm_topk")
    ens = split(recorded(w, monkeypatch, beams=3, ensemble=[w["A"], w["A2"]], ensemble_weights=[0.5, 0.5, 0.0],
                         ensemble_mode="logit")[2], "unimm_lm_topk")
    assert len(one) == len(ens) >= 4                                          # the same answers: the same number of steps
    for k in range(2, len(one)):
        side = one[k]
        assert side[0] == "unimm_kv_cache_update" and "unimm_lm_mix" not in side and "unimm_attn_decode" in side
        assert ens[k] == side[:1] * K + side[1:] * K + ["unimm_lm_mix"], k
    assert ens[1] == one[1] * K + ["unimm_lm_mix"] and ens[0][-1] == "unimm_lm_mix" and ens[0].count("unimm_lm_mix") == 1
