"""Speculative greedy answer generation on the GPU: `generate_answers(draft=...)` on the tiny model of tests/test_gpu_generate.py
against the float64 oracle and against the plain beams = 1 call, with three drafts -- A a frozen copy (acceptance near 1), B
another initialisation that shares the target's decoder bias (mixed acceptance: slots advance at different rates in one batch),
C the same without the bias (accepts the forced [SEP] only) -- and once on the full config."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests import test_gpu_generate as TG
from tests import test_gpu_generate_edges as TE

pytestmark = pytest.mark.gpu
SEP = 102
T, MAXLEN, G = 96, 12, 8
ROOT = TG.ROOT


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
    drafts = {"A": frozen_reference(model)}
    for name in ("B", "C"):
        sd2 = R.init_state_dict(ocfg, seed=12)
        if name == "B":
            sd2["cls.predictions.bias"] = sd["cls.predictions.bias"].clone()
        m = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd))
        m.load_state_dict(sd2, strict=True)
        drafts[name] = m.cuda().eval()
    d, c, utts = TG.make_dialogs(G, T, 1000, 37, 192, seed=22, cmin=8, cmax=60)
    limits = np.minimum(MAXLEN, (T - c) // 2 - 1)
    plain = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=1, max_answer_len=MAXLEN,
                                   **TG.gen_kwargs(d))
    torch.cuda.synchronize()
    return dict(model=model, ocfg=ocfg, sd=sd, drafts=drafts, d=d, c=c, utts=utts, limits=limits, plain=plain, oracle={}, spec={})


def spec_call(w, name, gamma):
    """one speculative call per (draft, draft_len), shared by the tests"""
    if (name, gamma) not in w["spec"]:
        d = w["d"]
        w["spec"][name, gamma] = w["model"].generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], w["c"], beams=1,
                                                             max_answer_len=MAXLEN, draft=w["drafts"][name], draft_len=gamma,
                                                             **TG.gen_kwargs(d))
        torch.cuda.synchronize()
    return w["spec"][name, gamma]


def oracle_rows(w, g, ans):
    """The teacher-forced float64 oracle's log p rows of dialog g's answer, with the step rules applied; computed once per
    (dialog, answer)."""
    key = (g, tuple(ans))
    if key not in w["oracle"]:
        lp = TG.oracle_steps(w["ocfg"], w["sd"], w["d"], [g], w["utts"], [list(ans)], T)[0]
        w["oracle"][key] = (lp, [TG.banned_row(lp[k], k, int(w["limits"][g])) for k in range(len(ans) + 1)])
    return w["oracle"][key]


def margin(row):
    top2 = torch.topk(row, 2).values
    return float(top2[0] - top2[1])


def shape_ok(res, limits):
    assert res.tokens.shape == (G, 1, MAXLEN + 1) and res.step_logp.shape == (G, 1, MAXLEN + 1)
    assert res.lengths.shape == res.scores.shape == res.logp.shape == (G, 1)
    for g in range(G):
        ans, n = TG.answers_of(res, g, 0)
        assert n >= 2 and res.tokens[g, 0, n - 1] == SEP and not set(ans) & {0, 101, 103, SEP} and not res.tokens[g, 0, n:].any()
        assert len(ans) <= limits[g]


@pytest.mark.parametrize("gamma", [1, 3, 12])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_oracle_match(w, name, gamma):
    """test_tiny_config_teacher_forced_against_oracle on the speculative result"""
    res = spec_call(w, name, gamma)
    shape_ok(res, w["limits"])
    clear = total = 0
    for g in range(G):
        ans, n = TG.answers_of(res, g, 0)
        lp, rows = oracle_rows(w, g, ans)
        toks = ans + [SEP]
        want = torch.stack([lp[k, t] for k, t in enumerate(toks)])
        got = res.step_logp[g, 0, :n].double().cpu()
        assert ((got - want).abs() <= 1e-2 + 1e-2 * want.abs()).all(), (g, got, want)
        assert abs(float(res.logp[g, 0]) - float(want.sum())) <= 1e-2 * n + 1e-2 * abs(float(want.sum()))
        assert float(res.scores[g, 0]) == float(res.logp[g, 0])
        for k, t in enumerate(toks):
            total += 1
            if margin(rows[k]) > 0.05:
                clear += 1
                assert int(torch.argmax(rows[k])) == t, (g, k)
    sp = res.speculation
    print(f"\ndraft {name}, draft_len {gamma}: {clear} of {total} steps clear; {sp.rounds} rounds, accepted "
          f"{int(sp.accepted.sum())} of {int(sp.drafted.sum())} drafts")
    assert clear >= 0.75 * total
    live = (sp.per_round >= 0).sum(0)
    assert torch.equal(sp.drafted, gamma * live) and torch.equal(sp.accepted, sp.per_round.clamp_min(0).sum(0))


@pytest.mark.parametrize("name,gamma", [("A", 3), ("B", 3), ("C", 1), ("A", 12)])
def test_against_plain_greedy(w, name, gamma):
    res, plain = spec_call(w, name, gamma), w["plain"]
    same = 0
    for g in range(G):
        a, b = TG.answers_of(res, g, 0)[0] + [SEP], TG.answers_of(plain, g, 0)[0] + [SEP]
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
        if k is None:
            assert a == b
            same += 1
            assert abs(float(res.logp[g, 0]) - float(plain.logp[g, 0])) <= 1e-3 * abs(float(plain.logp[g, 0])) + 1e-3
        else:                                   # tokens may only differ where the oracle cannot separate the top two
            assert margin(oracle_rows(w, g, b[:-1])[1][k]) <= 0.05, (g, k)
    print(f"\ndraft {name}, draft_len {gamma}: {same} of {G} dialogs identical to the plain beams = 1 call")


def test_mixed_acceptance(w):
    """draft B, draft_len 3: in some round two live dialogs accept different numbers of drafts"""
    sp = spec_call(w, "B", 3).speculation
    pr = sp.per_round.cpu()
    assert any(len(set(r[r >= 0].tolist())) > 1 for r in pr), pr
    assert 0 < int(sp.accepted.sum()) < int(sp.drafted.sum())
    print(f"\ndraft B: accepted per dialog {sp.accepted.tolist()} of {sp.drafted.tolist()} in {sp.rounds} rounds")


def rejections(res, gamma):
    """(dialog, step) of every draft the model rejected, from the per-round record: the round of dialog g that starts at n with a
    accepted drafts rejected the draft of step n + a, unless all were accepted or the round ended in an accepted [SEP]."""
    pr = res.speculation.per_round.cpu()
    out, acc = [], []
    for g in range(pr.shape[1]):
        n = 1
        for r in range(pr.shape[0]):
            a = int(pr[r, g])
            if a < 0:
                continue
            acc += [(g, n + j) for j in range(a)]
            if a < gamma and int(res.tokens[g, 0, n + a - 1]) != SEP:
                out.append((g, n + a))
            n += a + 1
    return out, acc


def test_high_and_low_acceptance(w):
    for gamma in (3, 12):
        res = spec_call(w, "A", gamma)
        rej, _ = rejections(res, gamma)
        for g, k in rej:                        # a copy of the model disagrees with it only where the top two are not separated
            ans = TG.answers_of(res, g, 0)[0]
            assert margin(oracle_rows(w, g, ans)[1][k]) <= 0.05, (g, k)
        assert int(res.speculation.accepted.sum()) > 0
    res = spec_call(w, "C", 3)
    _, acc = rejections(res, 3)
    for g, k in acc:                            # an unrelated draft is right only where the step rules leave one id
        assert k == w["limits"][g] and int(res.tokens[g, 0, k]) == SEP, (g, k)
    print(f"\ndraft A: {len(rej)} rejected drafts; draft C: {len(acc)} accepted, all forced [SEP]")


@pytest.mark.parametrize("cs,min_len", [(TE.LIMIT_CONTEXTS[3], 3), (TE.LIMIT_CONTEXTS[0], 0), ([23], 3)])
def test_mixed_limits(w, cs, min_len):
    """limits that differ inside one batch (0 included: [SEP] forced at step 0, the dialog never enters a round), and G = 1"""
    model = w["model"]
    d, c, utts = TE.exact_dialogs(cs, seed=50 + min_len)
    for name, gamma in (("B", 3), ("A", 2)):
        res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=1, max_answer_len=TE.MAXLEN,
                                     min_answer_len=min_len, draft=w["drafts"][name], draft_len=gamma, **TG.gen_kwargs(d))
        torch.cuda.synchronize()
        stats = [0, 0]
        TE.check_generation(model, w["ocfg"], w["sd"], d, c, utts, res, 1, min_len, stats)
        assert stats[0] >= 0.75 * stats[1]
        lim = np.minimum(TE.MAXLEN, (TE.T - c) // 2 - 1)
        assert (res.speculation.drafted.cpu().numpy()[lim == 0] == 0).all()


def test_no_side_effects(w):
    model, d, c, utts = w["model"], w["d"], w["c"], w["utts"]
    seq, _ = TG.completed(utts, [[200, 300]] * G, T)
    sargs = (seq["tokens"].cuda(), d["image_feat"].cuda(), d["image_loc"].cuda(), seq["labels"].cuda())
    skw = dict(token_type_ids=seq["segments"].cuda(), position_ids=seq["positions"].cuda(),
               attention_mask=seq["txt_attention_mask"].cuda(), co_attention_mask=seq["co_attention_mask"].cuda(),
               image_attention_mask=d["image_attention_mask"].cuda())
    draft = w["drafts"]["B"]
    before = [m.sequence_log_likelihood(*sargs, **skw)[0] for m in (model, draft)]
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=1, max_answer_len=MAXLEN, draft=draft,
                                 draft_len=4, **TG.gen_kwargs(d))
    after = [m.sequence_log_likelihood(*sargs, **skw)[0] for m in (model, draft)]
    again = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=1, max_answer_len=MAXLEN,
                                   **TG.gen_kwargs(d))
    torch.cuda.synchronize()
    assert res.speculation is not None and again.speculation is None
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    for f in ("tokens", "lengths", "scores", "logp", "step_logp"):
        assert torch.equal(getattr(again, f), getattr(w["plain"], f)), f
    assert model.training is False and draft.training is False


def test_plain_call_is_launch_for_launch_what_it_was(w, monkeypatch):
    """The kernel names and launch counts the launch profiler records for a plain call, and the C entry points it calls, are
    the same with and without unimm_amd.speculative imported -- and the plain call does not import it."""
    from unimm_amd import lib as L
    model, d, c = w["model"], w["d"], w["c"]
    calls = []
    real = L._call
    monkeypatch.setattr(L, "_call", lambda name, *a: (calls.append(name), real(name, *a))[1])

    def run():
        calls.clear()
        L.prof_enable(True)
        try:
            res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=1, max_answer_len=MAXLEN,
                                         **TG.gen_kwargs(d))
            torch.cuda.synchronize()
            prof = {k: v[2] for k, v in L.prof_collect().items()}
        finally:
            L.prof_enable(False)
        return res, prof, [n for n in calls if not n.startswith("unimm_prof")]

    saved = sys.modules.pop("unimm_amd.speculative", None)
    try:
        without = run()
        assert "unimm_amd.speculative" not in sys.modules
    finally:
        if saved is not None:
            sys.modules["unimm_amd.speculative"] = saved
    import unimm_amd.speculative  # noqa: F401
    with_ = run()
    assert without[1] == with_[1] and sum(without[1].values()) > 0
    assert without[2] == with_[2] and "unimm_attn_decode" in without[2]
    assert not {"unimm_attn_verify", "unimm_kv_cache_append"} & set(without[2])
    for f in ("tokens", "lengths", "scores", "logp", "step_logp"):
        assert torch.equal(getattr(without[0], f), getattr(with_[0], f)) and torch.equal(getattr(with_[0], f), getattr(w["plain"], f))


def test_full_config_once():
    """G = 8, T = 256, contexts 10 .. 200, max_answer_len 20, draft_len 4, a 2 + 1 + 1-layer random draft: scores within 2e-3
    of scale of sequence_log_likelihood of the completed sequences."""
    from oracle import vilbert_ref as R
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    model = BertForMultiModalPreTraining(BertConfig.from_json_file(TG.CFG_PATH))
    model.load_state_dict(R.init_state_dict(R.make_config(TG.CFG_PATH), seed=5), strict=True)
    model = model.cuda().eval()
    cfgd = json.load(open(TG.CFG_PATH))
    cfgd.update(num_hidden_layers=2, v_num_hidden_layers=1, t_biattention_id=[1], v_biattention_id=[0])
    torch.manual_seed(3)
    draft = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd)).cuda().eval()
    Gf, Tf = 8, 256
    d, c, utts = TG.make_dialogs(Gf, Tf, 30522, 37, 2048, seed=104, cmin=10, cmax=200)
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=1, max_answer_len=20, draft=draft,
                                 draft_len=4, **TG.gen_kwargs(d))
    torch.cuda.synchronize()
    answers = []
    for g in range(Gf):
        ans, n = TG.answers_of(res, g, 0)
        assert n >= 2 and res.tokens[g, 0, n - 1] == SEP and not set(ans) & {0, 101, 103, SEP}
        answers.append(ans)
    seq, _ = TG.completed(utts, answers, Tf)
    dev = "cuda"
    want, _ = model.sequence_log_likelihood(seq["tokens"].to(dev), d["image_feat"].to(dev), d["image_loc"].to(dev),
                                            seq["labels"].to(dev), average=False, token_type_ids=seq["segments"].to(dev),
                                            position_ids=seq["positions"].to(dev), attention_mask=seq["txt_attention_mask"].to(dev),
                                            co_attention_mask=seq["co_attention_mask"].to(dev),
                                            image_attention_mask=d["image_attention_mask"].to(dev))
    got, want = res.scores.reshape(-1).cpu(), want.cpu()
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    sp = res.speculation
    print(f"\nfull config, draft 2 + 1 + 1 layers: |scores - sequence_log_likelihood| {err:.3e} ({err / scale:.2e} of scale); "
          f"{sp.rounds} rounds, accepted {int(sp.accepted.sum())} of {int(sp.drafted.sum())}")
    assert err <= 2e-3 * scale
    assert math.isfinite(err) and sp.rounds >= 1
