"""The history rules of answer generation without a GPU: the numpy restatement (tests/constrain_ref.py) on hand-written cases,
beam_search / sample_search driven by the table model of tests/test_generate_cpu.py through the restatement and the engine's own
history bookkeeping (generation.track_history), the refused requests, and the refusals of the two C entry points."""
import ctypes

import numpy as np
import pytest
import torch

from tests import constrain_ref as CR
from tests.test_generate_cpu import NEG, VOCAB, TableModel, fake_step, topk
from tests.test_generate_sample_cpu import BANNED, draw, fake_sample_step
from unimm_amd import generation as GN

SEP = GN.SEP
V = 1000


# ---- the restatement on hand-written cases -------------------------------------------------------------------------------------
def test_overlapping_windows_count():
    assert CR.ban_set([5, 5], None, 2, V, SEP) == {5}                         # `a a`, n = 2: a is banned
    assert CR.ban_set([5, 6, 5, 6, 5], None, 2, V, SEP) == {6}                # a b a b a
    assert CR.ban_set([5, 6, 5, 6, 5], None, 3, V, SEP) == {6}
    assert CR.ban_set([5, 5, 5, 5], None, 3, V, SEP) == {5}
    assert CR.ban_set([5, 6, 7], None, 2, V, SEP) == set()


@pytest.mark.parametrize("n", [2, 3, 8])
def test_history_shorter_than_the_prefix_bans_nothing(n):
    ctx = [9] * 12
    assert CR.ban_set([9] * (n - 2), ctx, n, V, SEP) == set()                 # k = n - 2: nothing, from either source
    assert CR.ban_set([9] * (n - 1), ctx, n, V, SEP) == {9}                   # k = n - 1: the context's windows count
    assert CR.ban_set([9] * (n - 1), None, n, V, SEP) == set()                # ... the answer has no window of n tokens yet
    assert CR.ban_set([9] * n, None, n, V, SEP) == {9}                        # k = n


def test_unigrams_ban_every_id_of_the_sources():
    assert CR.ban_set([], None, 1, V, SEP) == set()
    assert CR.ban_set([], [4, 8, SEP, 4], 1, V, SEP) == {4, 8}
    assert CR.ban_set([7, 3], [4, 8, SEP, 4], 1, V, SEP) == {3, 4, 7, 8}
    assert CR.ban_set([7, 3], None, 1, V, SEP) == {3, 7}
    assert CR.ban_set([7], None, 0, V, SEP) == set()                          # n = 0 is off


def test_no_window_spans_the_context_answer_boundary():
    # context ends in 4, the answer starts with 6: `4 6` is no window, so a later 4 does not ban 6
    assert CR.ban_set([6, 4], [9, 4], 2, V, SEP) == set()
    assert CR.ban_set([6, 4], [4, 6], 2, V, SEP) == {6}                       # the same bigram inside the context does
    assert CR.ban_set([6, 7, 4], [9, 4], 3, V, SEP) == set()


def test_sep_is_never_banned_and_ids_outside_the_vocabulary_ban_nothing():
    assert CR.ban_set([5], [5, SEP, 5, 7], 2, V, SEP) == {7}
    assert CR.ban_set([], [SEP, SEP], 1, V, SEP) == set()
    assert CR.ban_set([5], [5, V, 5, -3, 5, V + 7], 2, V, SEP) == set()
    # an id outside [0, V) still compares as an integer: it can be part of a matching prefix
    assert CR.ban_set([V + 1], [V + 1, 6, V + 2, 7], 2, V, SEP) == {6}
    assert CR.ban_set([-1, 4], [-1, 4, 8, -2, 4, 9], 3, V, SEP) == {8}


def test_penalty_on_every_kind_of_logit():
    x = np.array([2.0, -2.0, 0.0, NEG, 3.0, -0.0, 1.5], dtype=np.float32)
    r = np.float32(1.3)
    inv = np.float32(1.0 / float(r))
    got = CR.penalised_row(x, [0, 1, 2], [3, 5, 99, -1], r, inv)
    assert got.dtype == np.float32
    want = np.array([np.float32(2.0) * inv, np.float32(-2.0) * r, 0.0, NEG, 3.0, -0.0, 1.5], dtype=np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert got[0] < x[0] and got[1] < x[1] and got[4] == x[4] and got[6] == x[6]   # r > 1 lowers both signs; others untouched
    assert np.array_equal(CR.penalised_row(x, [], None, r, inv).view(np.int32), x.view(np.int32))
    t = torch.from_numpy(x)                                                    # one fp32 multiply: a torch product gives the bits
    assert float(t[0] * torch.tensor(inv)) == float(got[0]) and float(t[1] * torch.tensor(r)) == float(got[1])


# ---- the searches, driven by the table model through the restatement and generation.track_history --------------------------------
def _row(model, g, a, flags, cons, ctx):
    """(log p with the step rules and the n-gram bans at -inf, the row selected by) of a slot whose answer so far is `a`."""
    lp = model.logp(g, a).copy()
    ban = CR.ban_set(a, ctx, cons["ngram"], 1 << 16, SEP)
    for i, t in enumerate(VOCAB):
        if t in BANNED or (t == SEP and flags & GN.SEP_BANNED) or (t != SEP and flags & GN.SEP_FORCED) or t in ban:
            lp[i] = NEG
    index = {t: i for i, t in enumerate(VOCAB)}
    r = np.float32(cons["penalty"])
    sel = CR.penalised_row(lp, [index.get(t, -1) for t in a], None if ctx is None else [index.get(t, -1) for t in ctx], r,
                           np.float32(1.0 / float(r)))
    return lp, sel


def _answers(hist):
    return [hist["hist"][s, :int(hist["len"][s])].tolist() for s in range(hist["hist"].shape[0])]


def constrained_step(model, G, beams, cons, width, contexts=None):
    hist = GN.new_history(G * beams, width)

    def step(k, parent, token, flags):
        GN.track_history(hist, k, token, parent)
        S = G * beams
        vals = torch.empty((S, beams), dtype=torch.float32)
        ids = torch.empty((S, beams), dtype=torch.int64)
        for s, a in enumerate(_answers(hist)):
            lp, sel = _row(model, s // beams, a, int(flags[s]), cons, None if contexts is None else contexts[s // beams])
            for r, (_, t) in enumerate(topk(sel, beams)):                        # ranked by the penalised row, valued by the raw one
                vals[s, r], ids[s, r] = float(lp[VOCAB.index(t)]), t
        return vals, ids

    return step


def constrained_sample_step(model, G, samples, seed, cons, width, contexts=None):
    hist = GN.new_history(G * samples, width)

    def step(k, token, flags):
        GN.track_history(hist, k, token)
        S = G * samples
        tok = torch.empty(S, dtype=torch.int64)
        lp_ = torch.empty(S, dtype=torch.float32)
        lq_ = torch.empty(S, dtype=torch.float32)
        for s, a in enumerate(_answers(hist)):
            lp, sel = _row(model, s // samples, a, int(flags[s]), cons, None if contexts is None else contexts[s // samples])
            t, _, lq = draw(sel, k, s, seed)
            tok[s], lp_[s], lq_[s] = t, float(lp[VOCAB.index(t)]), float(lq)
        return tok, lp_, lq_

    return step


def _finished(out):
    for g in range(out.lengths.shape[0]):
        for b in range(out.lengths.shape[1]):
            n = int(out.lengths[g, b])
            if n:
                toks = out.tokens[g, b, :n].tolist()
                assert toks[-1] == SEP and SEP not in toks[:-1]
                yield g, b, toks[:-1]


CONTEXTS = [[3, 4, SEP, 5, 3, 4, SEP], [7, SEP], [6, 6, 6, SEP, 3]]


@pytest.mark.parametrize("scope", ["answer", "dialog"])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("beams", [1, 3])
def test_beam_search_never_repeats_an_ngram(beams, n, scope):
    G, max_len = 3, 4
    # the table model has five free ids: with n = 1 the context may take one of them, or a 4-token answer cannot exist
    contexts = None if scope == "answer" else CONTEXTS if n > 1 else [[7, SEP]] * G
    found = 0
    for seed in range(3):
        cons = GN.check_constraints(n, 1.0, scope, beams)
        out = GN.beam_search(constrained_step(TableModel(seed), G, beams, cons, max_len, contexts), G, beams, [4, 4, 3], max_len, 1, 0.0)
        for g, b, ans in _finished(out):
            found += 1
            assert not CR.repeats_ngram(ans, n, None if contexts is None else contexts[g]), (seed, g, b, ans)
    assert found >= 3 * G


@pytest.mark.parametrize("n", [1, 2])
def test_the_unconstrained_searches_do_repeat(n):
    """... so the two tests around this one are not vacuous: over the same models the plain searches return repeated n-grams."""
    G, max_len, repeats = 3, 4, 0
    for seed in range(3):
        plain = GN.beam_search(fake_step(TableModel(seed), G, 3, BANNED), G, 3, [4, 4, 3], max_len, 1, 0.0)
        drawn = GN.sample_search(fake_sample_step(TableModel(seed), G, 4, seed, []), G, 4, [4, 4, 3], max_len, 1, 0.0)
        repeats += sum(CR.repeats_ngram(a, n) for out in (plain, drawn) for _, _, a in _finished(out))
    assert repeats > 0


@pytest.mark.parametrize("penalty", [1.0, 1.5])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_sample_search_never_repeats_an_ngram(n, penalty):
    G, N, max_len = 3, 4, 4
    cons = GN.check_constraints(n, penalty, "answer", 1)
    differ = 0
    for seed in range(3):
        out = GN.sample_search(constrained_sample_step(TableModel(seed), G, N, seed, cons, max_len), G, N, [4, 4, 3], max_len, 1, 0.0)
        answers = list(_finished(out))
        assert len(answers) == G * N
        for g, j, ans in answers:
            assert not CR.repeats_ngram(ans, n), (seed, g, j, ans)
        assert torch.isfinite(out.step_logq).all() and torch.isfinite(out.step_logp).all()
        differ += int((out.step_logq != out.step_logp).any())
    assert differ > 0


def test_dialog_scope_keeps_context_tokens_out_of_sampled_answers():
    G, N, max_len = 3, 3, 2
    contexts = [[3, SEP, 4, SEP], [7, SEP], [5, 5, SEP, 6]]
    cons = GN.check_constraints(1, 1.0, "dialog", 1)
    for seed in range(3):
        out = GN.sample_search(constrained_sample_step(TableModel(seed), G, N, seed, cons, max_len, contexts), G, N, [2, 2, 2],
                               max_len, 1, 0.0)
        for g, _, ans in _finished(out):
            assert ans and not set(ans) & set(contexts[g]) and len(set(ans)) == len(ans)


@pytest.mark.parametrize("beams", [1, 3])
def test_rules_that_cannot_bind_leave_beam_search_exactly_alone(beams):
    G, max_len = 3, 4
    cons = GN.check_constraints(8, 1.0, "dialog", beams)                       # n larger than any answer, r = 1
    assert cons is not None
    for seed in range(3):
        got = GN.beam_search(constrained_step(TableModel(seed), G, beams, cons, max_len, CONTEXTS), G, beams, [4, 3, 1], max_len, 1, 1.0)
        want = GN.beam_search(fake_step(TableModel(seed), G, beams, BANNED), G, beams, [4, 3, 1], max_len, 1, 1.0)
        for f in ("tokens", "lengths", "scores", "logp", "step_logp"):
            assert torch.equal(getattr(got, f), getattr(want, f)), f


def test_rules_that_cannot_bind_leave_sample_search_exactly_alone():
    G, N, max_len = 3, 4, 4
    cons = GN.check_constraints(8, 1.0, "answer", 1)
    for seed in range(3):
        got = GN.sample_search(constrained_sample_step(TableModel(seed), G, N, seed, cons, max_len), G, N, [4, 3, 1], max_len, 1, 1.0)
        want = GN.sample_search(fake_sample_step(TableModel(seed), G, N, seed, []), G, N, [4, 3, 1], max_len, 1, 1.0)
        for f in ("tokens", "lengths", "scores", "logp", "step_logp", "step_logq"):
            assert torch.equal(getattr(got, f), getattr(want, f)), f


def test_penalised_greedy_reports_the_raw_log_p():
    G, max_len = 3, 4
    cons = GN.check_constraints(0, 2.0, "answer", 1)
    changed = 0
    for seed in range(4):
        model = TableModel(seed)
        got = GN.beam_search(constrained_step(model, G, 1, cons, max_len), G, 1, [4, 4, 4], max_len, 1, 0.0)
        want = GN.beam_search(fake_step(model, G, 1, BANNED), G, 1, [4, 4, 4], max_len, 1, 0.0)
        changed += int(not torch.equal(got.tokens, want.tokens))
        for g, _, ans in _finished(got):
            toks = ans + [SEP]
            steps = [float(model.logp(g, toks[:k])[VOCAB.index(t)]) for k, t in enumerate(toks)]
            assert got.step_logp[g, 0, :len(toks)].tolist() == steps
    assert changed > 0


def test_track_history_follows_parents_and_clamps_its_width():
    h = GN.new_history(4, 2)
    assert h["hist"].dtype == torch.int32 and h["len"].dtype == torch.int32 and h["hist"].shape == (4, 2)
    GN.track_history(h, 0, torch.zeros(4, dtype=torch.int64), torch.arange(4))
    assert h["len"].tolist() == [0] * 4
    GN.track_history(h, 1, torch.tensor([5, 6, 7, 8]), torch.arange(4))
    GN.track_history(h, 2, torch.tensor([1, 2, 3, 4]), torch.tensor([3, 3, 0, 1]))
    assert h["hist"].tolist() == [[8, 1], [8, 2], [5, 3], [6, 4]] and h["len"].tolist() == [2] * 4
    GN.track_history(h, 3, torch.tensor([9, 9, 9, 9]), torch.tensor([0, 1, 2, 3]))     # past the width: kept, length clamped
    assert h["hist"].tolist() == [[8, 1], [8, 2], [5, 3], [6, 4]] and h["len"].tolist() == [2] * 4
    GN.track_history(h, 0, torch.zeros(4, dtype=torch.int64))
    assert h["len"].tolist() == [0] * 4
    GN.track_history(h, 1, torch.tensor([5, 6, 7, 8]))                                  # sampling: appended in place
    assert h["hist"][:, 0].tolist() == [5, 6, 7, 8] and h["len"].tolist() == [1] * 4


def test_context_table():
    ids = torch.tensor([[101, 5, 6, 102, 9, 9], [101, 7, 102, 3, 3, 3]])
    ctx, n = GN.context_table(ids, np.array([4, 3]))
    assert ctx.dtype == torch.int32 and n.dtype == torch.int32
    assert ctx.tolist() == [[5, 6, 102], [7, 102, 0]] and n.tolist() == [3, 2]


# ---- the refused requests --------------------------------------------------------------------------------------------------------
def test_check_constraints():
    assert GN.check_constraints() is None and GN.check_constraints(0, 1.0, "dialog", 4) is None
    assert GN.check_constraints(2, 1.0, "answer", 4) == dict(ngram=2, penalty=1.0, scope="answer")
    assert GN.check_constraints(np.int64(8), 1.5, "dialog", 1) == dict(ngram=8, penalty=1.5, scope="dialog")
    for n in (-1, 9, 2.0, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="no_repeat_ngram_size must be an integer in \\[0, 8\\]"):
            GN.check_constraints(n)
    for r in (0.0, -1.0, float("inf"), float("nan"), None, "1.2"):
        with pytest.raises(ValueError, match="repetition_penalty must be finite and > 0"):
            GN.check_constraints(0, r)
    for scope in ("question", "", None):
        with pytest.raises(ValueError, match="repeat_scope"):
            GN.check_constraints(2, 1.0, scope)
    with pytest.raises(ValueError, match="repetition_penalty = 1.2 needs beams = 1 .* different search"):
        GN.check_constraints(0, 1.2, "answer", 3)
    GN.check_constraints(0, 1.2, "answer", 1)


def test_generate_answers_refuses_before_the_engine_is_touched():
    import json
    import os
    from tests.test_generate_cpu import ROOT
    from unimm_amd import BertConfig, BertForMultiModalPreTraining, VisualDialogEncoder  # noqa: F401
    cfg = BertConfig.from_dict(json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json"))))
    ids = torch.zeros((1, 16), dtype=torch.int64)
    feat, loc = torch.zeros((1, 37, 192)), torch.zeros((1, 37, 5))
    model = BertForMultiModalPreTraining(cfg)
    for kw, match in ((dict(no_repeat_ngram_size=9), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"),
                      (dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
                      (dict(repeat_scope="turn", no_repeat_ngram_size=2), "repeat_scope"),
                      (dict(repetition_penalty=1.3, beams=2), "different search"),
                      (dict(repetition_penalty=1.3, samples=2, beams=2), "beams")):
        with pytest.raises(ValueError, match=match):
            model.generate_answers(ids, feat, loc, [4], **kw)
    with pytest.raises(NotImplementedError):                                   # the fp32x3 engine refuses as before
        BertForMultiModalPreTraining(cfg, compute_dtype="fp32x3").generate_answers(ids, feat, loc, [4], no_repeat_ngram_size=2)


# ---- the C entry points ----------------------------------------------------------------------------------------------------------
def test_hist_entry_points_refuse_before_any_launch():
    """unimm_lm_topk_hist / unimm_lm_sample_hist return before anything touches a device (no pointer is followed but the
    struct's): UNIMM_E_ARG (-1) for a NULL struct, a penalty that is not positive and finite, a rule without a history and a
    table without its lengths, UNIMM_E_SHAPE (-2) for ngram / ldh / ldc / nctx out of range; rows = 0 is OK."""
    from unimm_amd import build, lib
    build.build()
    L = lib.lib()
    P = 4096                                                                   # any non-NULL address

    def history(**kw):
        f = dict(hist=P, hist_len=P, ctx=None, ctx_len=None, ctx_idx=None, ldh=21, nctx=0, ldc=0, ngram=2, sep=102, penalty=1.0,
                 inv_penalty=1.0)
        f.update(kw)
        h = lib.LmHistory()
        for k, v in f.items():
            setattr(h, k, v)
        return h

    def topk(h, rows=0, V=30522, ldl=30522, K=4, vals=P):
        return L.unimm_lm_topk_hist(P, rows, V, ldl, None, 0, None, 102, K, None if h is None else ctypes.addressof(h), vals, P, None,
                                    None)

    def sample(h, rows=0, V=30522, ldl=30522, t=P, token=P):
        return L.unimm_lm_sample_hist(P, rows, V, ldl, None, 0, None, 102, t, P, P, 7, P, None if h is None else ctypes.addressof(h),
                                      token, P, P, None, None)

    for call in (topk, sample):
        assert call(history()) == 0 and call(history(ctx=P, ctx_len=P, ctx_idx=P, nctx=3, ldc=256, ldh=128, ngram=8)) == 0
        assert call(history(hist=None, hist_len=None, ngram=0)) == 0          # nothing on: no history needed
        assert call(history(penalty=1.3, inv_penalty=1 / 1.3, ngram=0)) == 0
        for rows in (0, 4):
            assert call(None, rows=rows) == -1
            for kw in (dict(penalty=0.0), dict(penalty=-1.0), dict(penalty=float("inf")), dict(penalty=float("nan")),
                       dict(inv_penalty=0.0), dict(inv_penalty=float("nan")), dict(inv_penalty=float("inf")),
                       dict(hist=None), dict(hist=None, ngram=0, penalty=1.3, inv_penalty=0.77), dict(hist_len=None),
                       dict(ctx=P), dict(ctx=P, ctx_len=P), dict(ctx=P, ctx_idx=P)):
                assert call(history(**kw), rows=rows) == -1, (call.__name__, kw)
            for kw in (dict(ngram=-1), dict(ngram=9), dict(ldh=129), dict(ldh=-1), dict(ctx=P, ctx_len=P, ctx_idx=P, nctx=0, ldc=8),
                       dict(ctx=P, ctx_len=P, ctx_idx=P, nctx=2, ldc=257), dict(ctx=P, ctx_len=P, ctx_idx=P, nctx=2, ldc=-1)):
                assert call(history(**kw), rows=rows) == -2, (call.__name__, kw)
    # the refusals of the plain entry points still hold
    assert topk(history(), vals=None) == -1 and topk(history(), K=17) == -2 and topk(history(), V=65537, ldl=65537) == -2
    assert sample(history(), t=None) == -1 and sample(history(), token=None) == -1 and sample(history(), ldl=30521) == -2
    assert lib.ABI_VERSION == 24 and {"unimm_lm_topk_hist", "unimm_lm_sample_hist"} <= set(lib.SYMBOLS)
    assert lib.STRUCTS["unimm_lm_history"] is lib.LmHistory
