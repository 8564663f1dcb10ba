"""Answer generation without a GPU: the beam driver of unimm_amd/generation.py against a table-driven fake model, the answer
position / segment rule against oracle.masks.encode_gen, and the refused requests."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from oracle import masks as OM
from unimm_amd import generation as GN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEP = GN.SEP
VOCAB = [0, 3, 4, 5, 6, 7, SEP, 103]          # V = 8 token ids (0 and 103 are banned by default)
NEG = float("-inf")


class TableModel:
    """log p of the next token given (dialog, prefix): seeded logits on a coarse grid (exact ties are common), cached."""

    def __init__(self, seed, grid=0.5, levels=4):
        self.seed, self.grid, self.levels, self.memo = seed, grid, levels, {}

    def logp(self, g, prefix):
        key = (g, tuple(prefix))
        if key not in self.memo:
            h = abs(hash((self.seed,) + key)) % (2 ** 32)
            x = np.random.default_rng(h).integers(0, self.levels, len(VOCAB)).astype(np.float32) * np.float32(self.grid)
            m = x.max()
            lse = np.float32(m + np.log(np.exp(x - m).sum(dtype=np.float32)))
            self.memo[key] = (x - lse).astype(np.float32)
        return self.memo[key]


def banned_row(lp, k, limit, min_len, banned):
    """The step-k rules of generation.py on one row of log p (no renormalisation)."""
    lp = lp.copy()
    for i, t in enumerate(VOCAB):
        if t in banned or (t == SEP and k < min_len) or (t != SEP and k >= limit):
            lp[i] = NEG
    return lp


def topk(lp, K):
    """Top K by (value desc, id asc) -> [(value, id)]."""
    order = sorted(range(len(VOCAB)), key=lambda i: (-lp[i], VOCAB[i]))
    return [(np.float32(lp[i]), VOCAB[i]) for i in order[:K]]


def fake_step(model, G, beams, banned):
    """The step function beam_search takes, backed by the table model (what unimm_lm_topk computes, restated)."""
    state = {}

    def step(k, parent, token, flags):
        S = G * beams
        if k == 0:
            prefixes = [[] for _ in range(S)]
        else:
            prefixes = [state["p"][int(parent[s])] + [int(token[s])] for s in range(S)]
        state["p"] = prefixes
        vals = torch.empty((S, beams), dtype=torch.float32)
        ids = torch.empty((S, beams), dtype=torch.int64)
        for s in range(S):
            lp = model.logp(s // beams, prefixes[s]).copy()
            f = int(flags[s])
            for i, t in enumerate(VOCAB):
                if t in banned or (t == SEP and f & GN.SEP_BANNED) or (t != SEP and f & GN.SEP_FORCED):
                    lp[i] = NEG
            for r, (v, t) in enumerate(topk(lp, beams)):
                vals[s, r], ids[s, r] = float(v), t
        return vals, ids

    return step


def reference_search(model, g, beams, limit, max_len, min_len, length_penalty, banned):
    """Plain-Python restatement of the search semantics for one dialog -> [(final score, logp, tokens incl. [SEP])]."""
    live = [(np.float32(0.0), [])]
    finished = []
    for k in range(max_len + 1):
        cands = []
        for slot, (cum, toks) in enumerate(live):
            lp = banned_row(model.logp(g, toks), k, limit, min_len, banned)
            for v, t in topk(lp, beams):
                cands.append((np.float32(cum + v), slot, t, toks))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        new_live = []
        for sc, slot, t, toks in cands:
            if len(new_live) == beams:
                break
            if sc == NEG:
                continue
            if t == SEP:
                if len(finished) < beams:
                    final = np.float32(sc / np.float32((k + 1) ** length_penalty))
                    finished.append((final, k, len(finished), sc, toks + [SEP]))
            else:
                new_live.append((sc, toks + [t]))
        live = new_live
        if len(finished) >= beams or not live:
            break
    finished.sort(key=lambda f: (-f[0], f[1], f[2]))
    return [(f[0], f[3], f[4]) for f in finished[:beams]]


CASES = [c for c in itertools.product([1, 2, 3, 4], [0, 1, 2], [1, 3, 4], [0.0, 1.0], [0, 1]) if c[1] <= c[2]]


@pytest.mark.parametrize("beams,min_len,max_len,length_penalty,seed", CASES)
def test_beam_search_equals_restatement(beams, min_len, max_len, length_penalty, seed):
    G = 3
    limits = np.array([max_len, max(min_len, max_len - 1), min(max_len, max(min_len, 1))])   # a short-context dialog too
    banned = (0, 103)
    model = TableModel(seed)
    out = GN.beam_search(fake_step(model, G, beams, banned), G, beams, limits, max_len, min_len, length_penalty)
    assert out.tokens.shape == (G, beams, max_len + 1) and out.lengths.shape == (G, beams)
    for g in range(G):
        want = reference_search(model, g, beams, int(limits[g]), max_len, min_len, length_penalty, banned)
        for b in range(beams):
            if b >= len(want):
                assert int(out.lengths[g, b]) == 0 and float(out.scores[g, b]) == NEG
                continue
            final, logp, toks = want[b]
            n = int(out.lengths[g, b])
            assert out.tokens[g, b, :n].tolist() == toks, (g, b)
            assert (out.tokens[g, b, n:] == 0).all()
            assert float(out.scores[g, b]) == float(final) and float(out.logp[g, b]) == float(logp), (g, b)
            steps = [model.logp(g, toks[:k])[VOCAB.index(toks[k])] for k in range(n)]
            assert out.step_logp[g, b, :n].tolist() == [float(v) for v in steps] and (out.step_logp[g, b, n:] == 0).all()
            assert toks[-1] == SEP and SEP not in toks[:-1] and not set(toks) & set(banned)
            assert min_len + 1 <= n <= limits[g] + 1


def test_ties_and_early_sep_are_exercised():
    """The case table above covers exact ties between candidates and [SEP] chosen before the limit."""
    ties = early = 0
    for seed in (0, 1):
        model = TableModel(seed)
        for g in range(3):
            for prefix in ([], [3], [4, 5]):
                lp = model.logp(g, prefix)
                ties += len(lp) - len(set(lp.tolist()))
        out = GN.beam_search(fake_step(model, 3, 3, (0, 103)), 3, 3, [4, 4, 4], 4, 0, 0.0)
        early += int(((out.lengths > 0) & (out.lengths < 5)).sum())
    assert ties > 0 and early > 0


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("min_len", [0, 2])
def test_greedy_is_argmax_walk(seed, min_len):
    G, max_len, banned = 4, 4, (0, 103)
    model = TableModel(seed, grid=0.37, levels=7)
    limits = np.array([4, 3, 2, 4])
    out = GN.beam_search(fake_step(model, G, 1, banned), G, 1, limits, max_len, min_len, 0.0)
    for g in range(G):
        toks, total = [], np.float32(0.0)
        for k in range(max_len + 1):
            v, t = topk(banned_row(model.logp(g, toks), k, int(limits[g]), min_len, banned), 1)[0]
            toks.append(t)
            total = np.float32(total + v)
            if t == SEP:
                break
        n = int(out.lengths[g, 0])
        assert out.tokens[g, 0, :n].tolist() == toks and float(out.logp[g, 0]) == float(total)


def test_answer_ids_follow_encode_gen():
    for utts, start in (([[5, 6], [7, 8, 9], [10, 11]], 0), ([[5], [7, 8], [12, 13], [4, 4, 4, 4]], 1), ([[9, 9, 9], [3]], 0)):
        enc = OM.encode_gen(utts, start_segment=start, max_seq_len=64)
        ans = utts[-1]
        n = len(ans) + 1
        L = int((enc["tokens"][0] != 0).sum()) - n
        c = L - n
        pos, seg = enc["positions"][0], enc["segments"][0]
        for k in range(n):
            p, s = GN.answer_ids(int(pos[c - 1]), int(seg[c - 1]), k)
            assert (p, s) == (int(pos[c + k]), int(seg[c + k])), k          # answer token k (the last one: [SEP])
            assert (p, s) == (int(pos[L + k]), int(seg[L + k])), k          # its [MASK] copy
            assert enc["labels"][0, L + k] == (ans + [SEP])[k]


def test_limits_and_refusals():
    assert GN.answer_limits([10, 200, 230, 250], 256, 30).tolist() == [30, 27, 12, 2]
    assert GN.check_request([10, 250], 256, 16, 20, 1).tolist() == [20, 2]
    with pytest.raises(ValueError, match="beams"):
        GN.check_request([10], 256, 17, 20, 1)
    with pytest.raises(ValueError, match="beams"):
        GN.check_request([10], 256, 0, 20, 1)
    with pytest.raises(ValueError, match="dialog 1"):
        GN.check_request([10, 253], 256, 4, 20, 1)                        # (256 - 253) // 2 - 1 = 0 tokens
    with pytest.raises(ValueError, match="dialog 0"):
        GN.check_request([250], 256, 4, 20, 3)
    with pytest.raises(ValueError, match="min_answer_len"):
        GN.check_request([10], 256, 1, 2, 3)


def _small_model(**over):
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    cfgd = json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json")))
    cfg = BertConfig.from_dict(cfgd)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def test_model_refuses_x3_and_no_coattention():
    from unimm_amd import BertForMultiModalPreTraining
    cfg = _small_model()
    ids = torch.zeros((1, 16), dtype=torch.int64)
    feat, loc = torch.zeros((1, 37, 192)), torch.zeros((1, 37, 5))
    with pytest.raises(NotImplementedError):
        BertForMultiModalPreTraining(cfg, compute_dtype="fp32x3").generate_answers(ids, feat, loc, [4])
    cfg2 = _small_model(with_coattention=False)
    with pytest.raises(NotImplementedError):
        BertForMultiModalPreTraining(cfg2).generate_answers(ids, feat, loc, [4])
    with pytest.raises(ValueError, match="beams"):
        BertForMultiModalPreTraining(cfg).generate_answers(ids, feat, loc, [4], beams=17)
    with pytest.raises(ValueError, match="room"):
        BertForMultiModalPreTraining(cfg).generate_answers(ids, feat, loc, [14])
