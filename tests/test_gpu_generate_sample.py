"""Sampled answer generation on the GPU: generate_answers(samples=...) against the CPU oracle (tiny config, teacher-forced),
against greedy decoding (samples = 1, top_k = 1), seeds and streams, no side effects, and against sequence_log_likelihood of the
completed sequences (full config).  The model and dialog builders are those of tests/test_gpu_generate.py."""
import math

import numpy as np
import pytest
import torch

from tests import sample_ref as SR
from tests.test_gpu_generate import (SEP, answers_of, banned_row, completed, full, gen_kwargs, make_dialogs, oracle_steps,  # noqa: F401
                                     tiny)

pytestmark = pytest.mark.gpu
T_TINY, G_TINY, MAXLEN, SAMPLES = 64, 6, 8, 4


def tiny_dialogs():
    return make_dialogs(G_TINY, T_TINY, 1000, 37, 192, seed=21, cmin=8, cmax=40)


def sample(model, d, c, **kw):
    kw.setdefault("samples", SAMPLES)
    kw.setdefault("max_answer_len", MAXLEN)
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, **gen_kwargs(d), **kw)
    torch.cuda.synchronize()
    return res


def flat(res, banned=(0, 101, 103)):
    """[(g, j, answer tokens, n)] with the invariants of every sampled answer."""
    out = []
    G, S = res.lengths.shape
    for g in range(G):
        for j in range(S):
            ans, n = answers_of(res, g, j)
            assert n >= 1 and res.tokens[g, j, n - 1] == SEP and not set(ans) & (set(banned) | {SEP})
            assert (res.tokens[g, j, n:] == 0).all() and (res.step_logp[g, j, n:] == 0).all() and (res.step_logq[g, j, n:] == 0).all()
            out.append((g, j, ans, n))
    return out


def test_tiny_config_teacher_forced_against_oracle(tiny):
    """Every step_logp within 1e-2 + 1e-2 |want| of the oracle's log p of the drawn token, logp within 1e-2 n + 1e-2 |sum| (the
    gates of tests/test_gpu_generate.py).  step_logq is the log-probability after renormalising over the ids the step leaves
    eligible, so it equals step_logp (to 1e-5) exactly where the step removes nothing -- checked with banned_tokens = (),
    min_answer_len = 0 on the steps before the dialog's limit; at the limit [SEP] is forced and logq = 0.  With the default
    banned ids logq >= logp."""
    model, ocfg, sd = tiny
    d, c, utts = tiny_dialogs()
    res = sample(model, d, c, temperature=1.0, seed=3)
    rows = flat(res)
    steps = oracle_steps(ocfg, sd, d, [g for g, _, _, _ in rows], utts, [a for _, _, a, _ in rows], T_TINY)
    for (g, j, ans, n), lp in zip(rows, steps):
        toks = ans + [SEP]
        want = torch.stack([lp[k, t] for k, t in enumerate(toks)])
        got = res.step_logp[g, j, :n].double().cpu()
        assert ((got - want).abs() <= 1e-2 + 1e-2 * want.abs()).all(), (g, j, got, want)
        assert abs(float(res.logp[g, j]) - float(want.sum())) <= 1e-2 * n + 1e-2 * abs(float(want.sum()))
        assert abs(float(res.scores[g, j]) - float(res.logp[g, j])) == 0.0                # length_penalty = 0
        assert (res.step_logq[g, j, :n] >= res.step_logp[g, j, :n] - 1e-5).all()
    free = sample(model, d, c, temperature=1.0, seed=3, banned_tokens=(), min_answer_len=0)
    compared = 0
    for g, j, ans, n in flat(free, banned=()):
        limit = min(MAXLEN, (T_TINY - int(c[g])) // 2 - 1)
        m = min(n, limit)                                                                  # steps that remove nothing
        assert (free.step_logq[g, j, :m] - free.step_logp[g, j, :m]).abs().max().item() <= 1e-5 if m else True
        if n == limit + 1:
            assert float(free.step_logq[g, j, n - 1]) == 0.0
        compared += m
    assert compared >= G_TINY * SAMPLES


def test_one_sample_top_k_1_is_greedy(tiny):
    model, _, _ = tiny
    d, c, _ = tiny_dialogs()
    greedy = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=1, max_answer_len=MAXLEN, **gen_kwargs(d))
    one = sample(model, d, c, samples=1, top_k=1, temperature=0.7, seed=9)
    assert torch.equal(one.tokens, greedy.tokens) and torch.equal(one.lengths, greedy.lengths)
    assert (one.step_logp - greedy.step_logp).abs().max().item() <= 1e-5
    assert (one.step_logq == 0).all()


def undecided_in_oracle(ocfg, sd, d, utts, c, g, prefix, k, seed, stream, temperature=1.0, margin=0.05):
    """Whether the oracle cannot separate the two best perturbed values of step k of dialog g after `prefix` (margin: the
    engine-against-oracle tolerance tests/test_gpu_generate.py uses for its top-2 checks)."""
    from unimm_amd import dropout as DR
    from unimm_amd import generation as GN
    lp = oracle_steps(ocfg, sd, d, [g], utts, [prefix], T_TINY)[0][k]
    row = banned_row(lp, k, min(MAXLEN, (T_TINY - int(c[g])) // 2 - 1)).numpy()
    ids = np.nonzero(row > -math.inf)[0]
    v = row[ids] / temperature + SR.gumbel64(DR.make_key(seed, k, GN.SAMPLE_SITE), stream, ids)
    top2 = np.sort(v)[-2:]
    return len(ids) > 1 and float(top2[1] - top2[0]) <= margin


def test_seeds_and_streams(tiny):
    model, ocfg, sd = tiny
    d, c, utts = tiny_dialogs()
    a = sample(model, d, c, seed=5)
    b = sample(model, d, c, seed=5)
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.step_logp, b.step_logp) and torch.equal(a.step_logq, b.step_logq)
    other = sample(model, d, c, seed=6)
    assert any(not torch.equal(a.tokens[g], other.tokens[g]) for g in range(G_TINY))
    for g in range(G_TINY):
        assert len({tuple(a.tokens[g, j].tolist()) for j in range(SAMPLES)}) > 1, (g, a.tokens[g])
    # the dialogs reversed with their streams: the reversed result, wherever the oracle's step distribution is decided
    rev = torch.arange(G_TINY - 1, -1, -1)
    dr = {k: v[rev] for k, v in d.items()}
    r = sample(model, dr, c[rev.numpy()], seed=5, sample_streams=rev)
    draws = int(a.lengths.sum())
    differ = 0
    for g in range(G_TINY):
        for j in range(SAMPLES):
            x, y = a.tokens[g, j].tolist(), r.tokens[G_TINY - 1 - g, j].tolist()
            if x != y:
                k = next(i for i, (p, q) in enumerate(zip(x, y)) if p != q)
                assert undecided_in_oracle(ocfg, sd, d, utts, c, g, x[:k], k, 5, g * SAMPLES + j), (g, j, k)
                differ += 1
    print(f"\nreversed batch: {differ} of {G_TINY * SAMPLES} samples differ ({draws} draws)")
    assert differ <= 1e-3 * draws
    # without sample_streams the draws follow the position in the batch instead
    pos = sample(model, dr, c[rev.numpy()], seed=5)
    assert not torch.equal(pos.tokens, r.tokens)


def test_no_side_effects(tiny):
    model, _, _ = tiny
    d, c, utts = tiny_dialogs()
    seq, _ = completed(utts, [[200, 300]] * G_TINY, T_TINY)
    sargs = (seq["tokens"].cuda(), d["image_feat"].cuda(), d["image_loc"].cuda(), seq["labels"].cuda())
    skw = dict(token_type_ids=seq["segments"].cuda(), position_ids=seq["positions"].cuda(),
               attention_mask=seq["txt_attention_mask"].cuda(), co_attention_mask=seq["co_attention_mask"].cuda(),
               image_attention_mask=d["image_attention_mask"].cuda())
    before, _ = model.sequence_log_likelihood(*sargs, **skw)
    sample(model, d, c, top_k=20, top_p=0.9, temperature=0.8, seed=1)
    after, _ = model.sequence_log_likelihood(*sargs, **skw)
    torch.cuda.synchronize()
    assert torch.equal(before, after)


def test_full_config_logp_equals_sequence_log_likelihood(full):
    model, _, _ = full
    T, G = 256, 7
    d, c, utts = make_dialogs(G, T, 30522, 37, 2048, seed=77, cmin=10, cmax=200)
    res = sample(model, d, c, max_answer_len=20, top_p=0.9, temperature=0.8, seed=2)
    rows = flat(res)
    gs = [g for g, _, _, _ in rows]
    seq, _ = completed([utts[g] for g in gs], [a for _, _, a, _ in rows], T)
    dev = "cuda"
    want, _ = model.sequence_log_likelihood(seq["tokens"].to(dev), d["image_feat"][gs].to(dev), d["image_loc"][gs].to(dev),
                                            seq["labels"].to(dev), token_type_ids=seq["segments"].to(dev),
                                            position_ids=seq["positions"].to(dev), attention_mask=seq["txt_attention_mask"].to(dev),
                                            co_attention_mask=seq["co_attention_mask"].to(dev),
                                            image_attention_mask=d["image_attention_mask"][gs].to(dev))
    got, want = res.logp.reshape(-1).cpu(), want.cpu()
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"\nG = {G}, samples = {SAMPLES}: logp {float(got.min()):.3f} .. {float(got.max()):.3f}, lengths "
          f"{int(res.lengths.min())} .. {int(res.lengths.max())}, |sampled - sequence_log_likelihood| {err:.3e} ({err / scale:.2e} of scale)")
    assert err <= 2e-3 * scale
