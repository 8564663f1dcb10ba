"""One rollout for self-critical training without a GPU: the greedy slot and the per-draw decoding parameters of
unimm_amd/generation.py against the table-driven fake model of tests/test_generate_cpu.py -- the greedy slot of
sample_search(greedy=True) is beam_search(beams=1), the samples are those of the call without it, per-draw parameter sequences
are the separate scalar calls -- and the refused requests."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_generate_cpu import NEG, ROOT, VOCAB, TableModel, fake_step
from tests.test_generate_sample_cpu import BANNED, draw, fake_sample_step
from unimm_amd import generation as GN

SEP = GN.SEP
SHAPES = [(0, 1), (0, 4), (1, 4), (2, 3), (3, 3)]      # (min_answer_len, max_answer_len)


def limits_of(min_len, max_len):
    """A dialog with the whole answer length, one a token short, one AT its limit as early as min_answer_len allows."""
    return np.array([max_len, max(min_len, max_len - 1), min(max_len, max(min_len, 1))])


def filtered_draw(lp, k, stream, seed, t, top_k, top_p):
    """One draw from a row of log p (-inf where banned) after top-k, temperature and nucleus filtering, the header's order:
    rank by (value desc, id asc), keep the first top_k, y = x / t, keep {x >= theta}, Gumbel-max -> (token, logp, logq).
    (1, 0, 1) is `draw` of tests/test_generate_sample_cpu.py on the same row."""
    elig = [i for i in range(len(VOCAB)) if lp[i] > NEG]
    order = sorted(elig, key=lambda i: (-lp[i], VOCAB[i]))
    kept = order[:top_k] if top_k > 0 else order
    y = (lp / np.float32(t)).astype(np.float32)
    if top_p < 1.0:
        q = np.exp(y[kept].astype(np.float64) - float(y[kept[0]]))
        theta = next(lp[i] for i in kept if q[[lp[j] >= lp[i] for j in kept]].sum() >= float(np.float32(top_p)) * q.sum())
        kept = [i for i in kept if lp[i] >= theta]
    masked = np.full(len(VOCAB), NEG, dtype=np.float32)
    masked[kept] = y[kept]
    tok, _, lq = draw(masked, k, stream, seed)
    return tok, np.float32(lp[VOCAB.index(tok)]), lq


def rows_step(model, G, slots, seed, params, streams, calls=None):
    """The step function sample_search takes with PER-SLOT decoding parameters (what unimm_lm_sample_rows computes, restated):
    params = (temperature, top_k, top_p) [G * slots] as GN.slot_parameters lays them out, streams [G * slots]."""
    state = {}
    ts, ks, ps = params

    def step(k, token, flags):
        if calls is not None:
            calls.append(k)
        S = G * slots
        state["p"] = [[] for _ in range(S)] if k == 0 else [state["p"][s] + [int(token[s])] for s in range(S)]
        tok = torch.empty(S, dtype=torch.int64)
        lp_ = torch.empty(S, dtype=torch.float32)
        lq_ = torch.empty(S, dtype=torch.float32)
        for s in range(S):
            lp = model.logp(s // slots, state["p"][s]).copy()
            f = int(flags[s])
            for i, t in enumerate(VOCAB):
                if t in BANNED or (t == SEP and f & GN.SEP_BANNED) or (t != SEP and f & GN.SEP_FORCED):
                    lp[i] = NEG
            tok[s], lp_[s], lq_[s] = (float(v) for v in filtered_draw(lp, k, int(streams[s]), seed, float(ts[s]), int(ks[s]),
                                                                      float(ps[s])))
        return tok, lp_, lq_

    return step


def slot_streams(G, N, greedy):
    """Sample j of dialog g keeps stream g * N + j whether or not the greedy slot (stream 0: it decides nothing) is there."""
    st = np.arange(G)[:, None] * N + np.arange(N)[None]
    if greedy:
        st = np.concatenate([st, np.zeros((G, 1), dtype=np.int64)], 1)
    return st.reshape(-1)


def fused(model, G, N, seed, min_len, max_len, length_penalty, temperature=1.0, top_k=0, top_p=1.0, greedy=True, calls=None):
    ts, ks, ps, _ = GN.check_sampling(N, 1, temperature, top_k, top_p, greedy)
    params = GN.slot_parameters(G, ts, ks, ps, greedy)
    step = rows_step(model, G, N + greedy, seed, params, slot_streams(G, N, greedy), calls)
    return GN.sample_search(step, G, N, limits_of(min_len, max_len), max_len, min_len, length_penalty, greedy=greedy)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


@pytest.mark.parametrize("N", [1, 15])
@pytest.mark.parametrize("min_len,max_len", SHAPES)
@pytest.mark.parametrize("length_penalty", [0.0, 1.0])
def test_greedy_slot_is_beam_search_and_samples_are_the_plain_call(N, min_len, max_len, length_penalty):
    G, seed = 3, 11 + N
    model = TableModel(seed)
    calls = []
    out = fused(model, G, N, seed, min_len, max_len, length_penalty, calls=calls)
    limits = limits_of(min_len, max_len)
    beam = GN.beam_search(fake_step(model, G, 1, BANNED), G, 1, limits, max_len, min_len, length_penalty)
    gr = out.greedy
    assert gr is not None and gr.step_logq is None and gr.greedy is None
    for f in ("tokens", "lengths", "step_logp", "scores", "logp"):
        assert same(getattr(gr, f), getattr(beam, f)), (f, getattr(gr, f), getattr(beam, f))
    assert gr.tokens.shape == (G, 1, max_len + 1) and (gr.lengths >= min_len + 1).all()
    assert (gr.lengths[:, 0] <= torch.from_numpy(limits) + 1).all()
    plain = GN.sample_search(fake_sample_step(model, G, N, seed, []), G, N, limits, max_len, min_len, length_penalty)
    assert plain.greedy is None
    for f in ("tokens", "lengths", "step_logp", "step_logq", "scores", "logp"):
        assert same(getattr(out, f), getattr(plain, f)), f
        assert getattr(out, f).is_contiguous()
    assert out.tokens.shape == (G, N, max_len + 1)
    # the loop ends with the last slot's [SEP], the greedy one included
    assert calls == list(range(int(max(out.lengths.max(), gr.lengths.max()))))


def test_the_loop_waits_for_the_greedy_slot():
    """Over a few models the greedy answer is sometimes the longest of its batch: the loop must not stop before it ends."""
    longer = 0
    for seed in range(6):
        model = TableModel(seed)
        calls = []
        out = fused(model, 3, 1, seed, 0, 4, 0.0, calls=calls)
        assert (out.greedy.lengths > 0).all() and (out.greedy.tokens.gather(2, (out.greedy.lengths - 1)[:, :, None]) == SEP).all()
        longer += int(out.greedy.lengths.max() > out.lengths.max())
        assert len(calls) == int(max(out.lengths.max(), out.greedy.lengths.max()))
    assert longer > 0


def test_one_synchronisation_per_step_with_the_greedy_slot(monkeypatch):
    reads, inside = [], [False]
    for name in ("__bool__", "item", "tolist", "__int__", "__float__", "__index__", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **kw):
            if inside[0]:
                return _orig(self, *a, **kw)
            reads.append(_name)
            inside[0] = True
            try:
                return _orig(self, *a, **kw)
            finally:
                inside[0] = False

        monkeypatch.setattr(torch.Tensor, name, counted)
    G, N, seed = 3, 2, 1
    model, calls = TableModel(seed), []
    ts, ks, ps, _ = GN.check_sampling(N, 1, 1.0, 0, 1.0, True)
    inner = rows_step(model, G, N + 1, seed, GN.slot_parameters(G, ts, ks, ps, True), slot_streams(G, N, True), calls)

    def step(k, token, flags):
        inside[0] = True
        try:
            return inner(k, token, flags)
        finally:
            inside[0] = False

    GN.sample_search(step, G, N, np.array([4, 4, 3]), 4, 1, 1.0, greedy=True)
    assert len(calls) >= 2 and reads == ["__bool__"] * len(calls), (calls, reads)


@pytest.mark.parametrize("greedy", [False, True])
def test_per_draw_sequences_equal_the_scalar_calls(greedy):
    G, N, seed, min_len, max_len = 3, 4, 3, 1, 4
    temps, ks, ps = [1.0, 0.7, 2.0, 0.7], [0, 2, 3, 1], [1.0, 0.9, 0.5, 1.0]
    model = TableModel(seed)
    out = fused(model, G, N, seed, min_len, max_len, 1.0, temps, ks, ps, greedy)
    differ = 0
    for j in range(N):
        one = fused(model, G, N, seed, min_len, max_len, 1.0, temps[j], ks[j], ps[j], greedy)
        for f in ("tokens", "lengths", "step_logp", "step_logq", "scores", "logp"):
            assert same(getattr(out, f)[:, j], getattr(one, f)[:, j]), (j, f)
        differ += int(not same(out.tokens, one.tokens))
        if greedy:                                                    # the greedy slot does not see the draws' parameters
            for f in ("tokens", "lengths", "step_logp", "scores", "logp"):
                assert same(getattr(out.greedy, f), getattr(one.greedy, f)), (j, f)
    assert differ > 0                                                 # the parameters matter: the comparison is not vacuous
    # draw 3 has top_k = 1: the greedy answer, log q = 0 on every token
    if greedy:
        assert same(out.tokens[:, 3:4], out.greedy.tokens) and same(out.step_logp[:, 3:4], out.greedy.step_logp)
    assert (out.step_logq[:, 3] == 0).all()
    # one sequence among scalars is enough, and a tensor or an array is a sequence
    mixed = fused(model, G, N, seed, min_len, max_len, 1.0, torch.tensor(temps), 0, 1.0, greedy)
    only_t = fused(model, G, N, seed, min_len, max_len, 1.0, np.asarray(temps), [0] * N, (1.0,) * N, greedy)
    assert same(mixed.tokens, only_t.tokens) and same(mixed.step_logq, only_t.step_logq)


def test_check_sampling_and_slot_parameters():
    ts, ks, ps, per = GN.check_sampling(3, 1, 0.7, 5, 0.9)
    assert not per and ts.dtype == np.float32 and ks.dtype == np.int32 and ps.dtype == np.float32
    assert ts.tolist() == [np.float32(0.7)] * 3 and ks.tolist() == [5] * 3 and ps.tolist() == [np.float32(0.9)] * 3
    ts, ks, ps, per = GN.check_sampling(3, 1, [1.0, 0.5, 2.0], 5, 0.9, True)
    assert per and ts.tolist() == [1.0, 0.5, 2.0]
    t2, k2, p2 = GN.slot_parameters(2, ts, ks, ps, True)
    assert t2.tolist() == [1.0, 0.5, 2.0, 1.0] * 2 and k2.tolist() == [5, 5, 5, 1] * 2
    assert p2.tolist() == [np.float32(0.9)] * 3 + [1.0] + [np.float32(0.9)] * 3 + [1.0]
    assert t2.dtype == np.float32 and k2.dtype == np.int32 and p2.dtype == np.float32
    t2, k2, p2 = GN.slot_parameters(2, ts, ks, ps)
    assert t2.tolist() == [1.0, 0.5, 2.0] * 2 and len(k2) == len(p2) == 6
    for kw, match in ((dict(temperature=[1.0, 0.0, 1.0]), "temperature must be positive and finite, got 0.0"),
                      (dict(temperature=[1.0, 1.0, float("inf")]), "temperature"),
                      (dict(top_k=[0, 1, -1]), "top_k must be an integer >= 0"), (dict(top_k=[0, 1.5, 2]), "top_k"),
                      (dict(top_p=[1.0, 0.0, 0.5]), r"top_p must be in \(0, 1\]"), (dict(top_p=[1.0, 1.5, 0.5]), "top_p"),
                      (dict(temperature=[1.0, 1.0]), "2 temperature values for 3 samples"),
                      (dict(top_k=[1, 2, 3, 4]), "4 top_k values"), (dict(top_p=[]), "0 top_p values")):
        args = dict(temperature=1.0, top_k=0, top_p=1.0)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            GN.check_sampling(3, 1, args["temperature"], args["top_k"], args["top_p"])
    GN.check_sampling(15, 1, 1.0, 0, 1.0, True)
    GN.check_sampling(16, 1, 1.0, 0, 1.0, False)
    with pytest.raises(ValueError, match="32 query rows"):
        GN.check_sampling(16, 1, 1.0, 0, 1.0, True)


def test_rollout_refusals():
    from unimm_amd import BertConfig, BertForMultiModalPreTraining, trainer
    cfg = BertConfig.from_dict(json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json"))))
    ids = torch.zeros((1, 16), dtype=torch.int64)
    feat, loc = torch.zeros((1, 37, 192)), torch.zeros((1, 37, 5))
    model = BertForMultiModalPreTraining(cfg)
    with pytest.raises(ValueError, match="beams=1"):                   # greedy alone is beam search with one beam
        model.generate_answers(ids, feat, loc, [4], greedy=True)
    with pytest.raises(ValueError, match="beams=1"):
        GN.sample_search(None, 1, 0, [4], 4, greedy=True)
    with pytest.raises(ValueError, match="unimm_attn_decode takes .* 32 query rows per dialog"):
        model.generate_answers(ids, feat, loc, [4], samples=16, greedy=True)
    with pytest.raises(ValueError, match="samples"):
        model.generate_answers(ids, feat, loc, [4], samples=17, greedy=True)
    with pytest.raises(ValueError, match="beams"):
        model.generate_answers(ids, feat, loc, [4], samples=2, beams=2, greedy=True)
    with pytest.raises(ValueError, match="temperature"):
        model.generate_answers(ids, feat, loc, [4], samples=2, temperature=[1.0, -1.0])
    with pytest.raises(ValueError, match="top_p"):
        model.generate_answers(ids, feat, loc, [4], samples=2, top_p=[1.0, 0.0], greedy=True)
    with pytest.raises(ValueError, match="top_k"):
        model.generate_answers(ids, feat, loc, [4], samples=2, top_k=[1, 2, 3])
    for kw in (dict(samples=2, greedy=True), dict(samples=2, temperature=[1.0, 0.5]), dict(greedy=True)):
        with pytest.raises(NotImplementedError):                       # the fp32x3 engine refuses as before
            BertForMultiModalPreTraining(cfg, compute_dtype="fp32x3").generate_answers(ids, feat, loc, [4], **kw)
    for kw, match in ((dict(baseline="mean"), "baseline='greedy'"), (dict(baseline=None), "baseline='greedy'"),
                      (dict(baseline=torch.zeros(1)), "baseline='greedy'")):
        with pytest.raises(ValueError, match=match):                   # refused before the model is touched
            trainer.self_critical_step(None, None, None, {}, {}, 0, None, samples=2, rollout="fused", **kw)
    with pytest.raises(ValueError, match="rollout"):
        trainer.self_critical_step(None, None, None, {}, {}, 0, None, samples=2, rollout="both")


def test_lm_sample_rows_refuses_before_any_launch():
    """unimm_lm_sample_rows returns before anything touches a device (the pointers are never followed): a NULL parameter array or
    a NULL pointer of unimm_lm_sample's is UNIMM_E_ARG (-1), a bad shape UNIMM_E_SHAPE (-2), rows = 0 is OK."""
    from unimm_amd import build, lib
    build.build()
    f = lib.lib().unimm_lm_sample_rows
    P = 4096                                                           # any non-NULL address

    def call(rows=0, V=30522, ldl=30522, t=P, k=P, p=P, streams=P, token=P, banned=None, nbanned=0):
        return f(P, rows, V, ldl, banned, nbanned, None, 102, t, k, p, 7, streams, token, P, P, None, None)

    assert call() == 0 and call(V=65536, ldl=65536) == 0
    for kw in (dict(t=None), dict(k=None), dict(p=None), dict(streams=None), dict(token=None), dict(nbanned=3),
               dict(t=None, rows=4), dict(k=None, rows=4), dict(p=None, rows=4)):
        assert call(**kw) == -1, kw
    for kw in (dict(V=0), dict(V=65537, ldl=65537), dict(ldl=30521), dict(rows=-1), dict(nbanned=-1)):
        assert call(**kw) == -2, kw
    assert lib.ABI_VERSION == 24 and "unimm_lm_sample_rows" in lib.SYMBOLS
