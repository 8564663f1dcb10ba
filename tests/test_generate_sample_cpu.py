"""Sampled answer generation without a GPU: the sampling driver of unimm_amd/generation.py against a table-driven fake model, the
float32 restatement of unimm_lm_sample against the float64 one inside the budgets of tests/sample_ref.py (whose measured
constants this prints), the mirrored generator against the softmax, and the refused requests."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import generate_ref as GR
from tests import sample_ref as SR
from tests.test_generate_cpu import NEG, ROOT, VOCAB, TableModel, banned_row
from unimm_amd import generation as GN

SEP = GN.SEP
BANNED = (0, 103)


def draw(lp, k, stream, seed):
    """One draw from a row of log p with -inf where banned (Gumbel-max with the mirrored uniforms) -> (token, logp, logq)."""
    elig = np.nonzero(lp > NEG)[0]
    g = SR.gumbel64(SR.stream_key(seed, k), stream, np.asarray(VOCAB)[elig])
    i = int(elig[np.argmax(lp[elig].astype(np.float64) + g)])
    m = lp[elig].max()
    lq = np.float32(lp[i] - (m + np.log(np.exp(lp[elig] - m).sum(dtype=np.float32))))
    return VOCAB[i], np.float32(lp[i]), lq


def fake_sample_step(model, G, samples, seed, calls):
    """The step function sample_search takes, backed by the table model."""
    state = {}

    def step(k, token, flags):
        calls.append(k)
        S = G * samples
        state["p"] = [[] for _ in range(S)] if k == 0 else [state["p"][s] + [int(token[s])] for s in range(S)]
        tok = torch.empty(S, dtype=torch.int64)
        lp_ = torch.empty(S, dtype=torch.float32)
        lq_ = torch.empty(S, dtype=torch.float32)
        for s in range(S):
            lp = model.logp(s // samples, state["p"][s]).copy()
            f = int(flags[s])
            for i, t in enumerate(VOCAB):
                if t in BANNED or (t == SEP and f & GN.SEP_BANNED) or (t != SEP and f & GN.SEP_FORCED):
                    lp[i] = NEG
            tok[s], lp_[s], lq_[s] = (float(v) for v in draw(lp, k, s, seed))
        return tok, lp_, lq_

    return step


def reference_sample(model, g, j, samples, limit, max_len, min_len, seed):
    """Plain-Python walk of one slot -> (tokens incl. [SEP], step log p, step log q)."""
    toks, lps, lqs = [], [], []
    for k in range(max_len + 1):
        t, lp, lq = draw(banned_row(model.logp(g, toks), k, limit, min_len, BANNED), k, g * samples + j, seed)
        toks.append(t); lps.append(lp); lqs.append(lq)
        if t == SEP:
            break
    return toks, lps, lqs


@pytest.mark.parametrize("samples", [1, 3, 4])
@pytest.mark.parametrize("min_len,max_len", [(0, 1), (0, 4), (1, 4), (2, 3), (3, 3)])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0])
def test_sample_search_equals_restatement(samples, min_len, max_len, length_penalty):
    G, seed = 3, 5 + samples
    limits = np.array([max_len, max(min_len, max_len - 1), min(max_len, max(min_len, 1))])
    model = TableModel(seed)
    calls = []
    out = GN.sample_search(fake_sample_step(model, G, samples, seed, calls), G, samples, limits, max_len, min_len, length_penalty)
    assert out.tokens.shape == (G, samples, max_len + 1) and out.step_logq.shape == out.step_logp.shape == out.tokens.shape
    longest = 0
    for g in range(G):
        for j in range(samples):                                   # draw order: sample j of dialog g is stream g * samples + j
            toks, lps, lqs = reference_sample(model, g, j, samples, int(limits[g]), max_len, min_len, seed)
            n = int(out.lengths[g, j])
            longest = max(longest, n)
            assert out.tokens[g, j, :n].tolist() == toks and (out.tokens[g, j, n:] == 0).all(), (g, j)
            assert toks[-1] == SEP and SEP not in toks[:-1] and not set(toks) & set(BANNED)
            assert min_len + 1 <= n <= limits[g] + 1
            assert out.step_logp[g, j, :n].tolist() == [float(v) for v in lps] and (out.step_logp[g, j, n:] == 0).all()
            assert out.step_logq[g, j, :n].tolist() == [float(v) for v in lqs] and (out.step_logq[g, j, n:] == 0).all()
            total = out.step_logp[g, j].sum()
            assert float(out.logp[g, j]) == float(total)
            assert float(out.scores[g, j]) == float(total / torch.tensor(float(n)) ** length_penalty)
    assert calls == list(range(longest))                           # the loop ends with the last slot's [SEP]


def test_early_sep_and_different_samples_are_exercised():
    early = differ = 0
    for seed in range(4):
        model = TableModel(seed)
        out = GN.sample_search(fake_sample_step(model, 3, 4, seed, []), 3, 4, [4, 4, 4], 4, 0, 0.0)
        early += int((out.lengths < 5).sum())
        differ += sum(len({tuple(out.tokens[g, j].tolist()) for j in range(4)}) > 1 for g in range(3))
    assert early > 0 and differ > 0


def test_one_synchronisation_per_step(monkeypatch):
    """Outside the step function the driver reads a tensor's value exactly once per step (the `all finished` flag)."""
    reads = []
    inside = [False]
    for name in ("__bool__", "item", "tolist", "__int__", "__float__", "__index__", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **kw):
            if not inside[0]:
                reads.append(_name)
                inside[0] = True
                try:
                    return _orig(self, *a, **kw)
                finally:
                    inside[0] = False
            return _orig(self, *a, **kw)

        monkeypatch.setattr(torch.Tensor, name, counted)
    model, calls = TableModel(1), []
    inner = fake_sample_step(model, 3, 2, 1, calls)

    def step(k, token, flags):
        inside[0] = True
        try:
            return inner(k, token, flags)
        finally:
            inside[0] = False

    GN.sample_search(step, 3, 2, np.array([4, 4, 3]), 4, 1, 0.0)
    assert len(calls) >= 2 and reads == ["__bool__"] * len(calls), (calls, reads)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SR.SAMPLE_V)
def test_f32_restatement_inside_budgets(V):
    """The float32 restatement of every launch of the GPU suite (tests/test_gpu_generate_sample_edges.py) passes the checks the
    kernel's outputs get; prints the measured ratios the constants of tests/sample_ref.py come from."""
    case = SR.sample_case(V)
    rows = SR.case_rows(case)
    lse32 = GR.lm_lse_f32(case["x"], V).numpy().astype(np.float32)
    worst = np.zeros(3)
    draws = undecided = 0
    for k, p, t in SR.combos(V):
        tok = np.zeros(len(rows), dtype=np.int64)
        lq = np.zeros(len(rows), dtype=np.float32)
        lp = np.zeros(len(rows), dtype=np.float32)
        for r, row in enumerate(rows):
            r32 = SR.sample_row_f32(row, t, k, p)
            worst = np.maximum(worst, SR.measure_row(row, t, k, p, r32))
            tok[r], lq[r] = r32["token"], r32["logq"]
            lp[r] = np.float32(row.xall[tok[r]]) - lse32[r] if tok[r] >= 0 else -np.inf
        d, u, _ = SR.check_rows(rows, V, t, k, p, tok, lp, lq, lse32, what=f"V {V} top_k {k} top_p {p} t {t}")
        draws, undecided = draws + d, undecided + u
    print(f"\nV = {V}: worst float32 / float64 ratios: draw {worst[0]:.3f} (recorded {SR.DRAW_MEASURED}, C_DRAW {SR.C_DRAW}), "
          f"nucleus {worst[1]:.3f} (recorded {SR.NUC_MEASURED}, C_NUC {SR.C_NUC}), logq {worst[2]:.3f} (recorded {SR.Q_MEASURED}, "
          f"C_Q {SR.C_Q}); {undecided} of {draws} draws undecided")
    assert worst[0] <= SR.DRAW_MEASURED * 1.001 and worst[1] <= SR.NUC_MEASURED * 1.001 and worst[2] <= SR.Q_MEASURED * 1.001
    assert SR.C_DRAW == SR.pow2_at_least(8 * SR.DRAW_MEASURED) and SR.C_NUC == SR.pow2_at_least(8 * SR.NUC_MEASURED)
    assert SR.C_Q == SR.pow2_at_least(8 * SR.Q_MEASURED)
    assert undecided <= 1e-3 * draws


def test_planted_rows_do_what_they_are_planted_for():
    case = SR.sample_case(257)
    rows = SR.case_rows(case)
    name = {n: i for i, n in enumerate(case["names"])}
    r = rows[name["plateau on top"]]
    npl = int((r.x32 == 30.0).sum())
    assert npl > 50 and (r.x32[:npl] == 30.0).all()                   # top_k = 2 and 50 both cut inside the plateau,
    assert (np.diff(r.ids[:npl]) > 0).all()                           # where the id decides
    assert SR.sample_row(r, 1.0, 2, 1.0)["token"] in r.ids[:2].tolist()
    r = rows[name["plateau at the nucleus threshold"]]
    for t in SR.TEMPS:
        for p in (0.9, 0.5):
            assert SR.sample_row(r, t, 0, p)["lengths"] == [9]      # the top id and all eight tied ids
    assert SR.sample_row(r, 1.0, 0, 1e-6)["lengths"] == [1]
    for n in ("everything banned", "all -inf", "all -inf, sep forced"):
        assert rows[name[n]].n == 0 and SR.sample_row(rows[name[n]], 1.0, 0, 1.0)["token"] == -1
    assert rows[name["sep forced"]].ids.tolist() == [SR.SEP]
    assert SR.SEP not in rows[name["sep banned"]].ids
    banned = set(int(b) for b in case["banned"] if 0 <= b < 257)
    assert not banned & set(rows[name["banned ids on top"]].ids.tolist()) and len(case["banned"]) > len(banned)
    r = rows[name["signed zeros"]]
    z = np.nonzero(r.x32 == 0.0)[0]
    assert len(z) == 2 and r.ids[z[0]] < r.ids[z[1]]                  # -0 and +0 tie: by id


@pytest.mark.parametrize("V,streams,seed", [(16, 32768, 0), (16, 32768, 1), (257, 65536, 0)])
def test_mirrored_generator_follows_the_softmax(V, streams, seed):
    chi2, df, small, gmin = SR.chi_square(V, streams, seed=seed)
    print(f"\nV = {V}, {streams} streams: chi^2 {chi2:.1f} on {df} degrees of freedom (0.1 % critical value "
          f"{SR.chi_square_critical(df):.1f}); {small} draws with a top-2 gap below 1e-4, smallest {gmin:.2e}")
    assert chi2 < SR.chi_square_critical(df)
    assert small <= 1e-3 * streams


def test_uniforms_are_exact_and_inside_the_unit_interval():
    from unimm_amd.dropout import mix32_int
    ids = np.arange(1000)
    h = SR.hashes(0xDEADBEEF, -3, ids)
    sk = mix32_int(0xDEADBEEF ^ (((-3 & 0xFFFFFFFF) * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF))
    assert [int(v) for v in h[:50]] == [mix32_int((sk + i * 0x85EBCA77) & 0xFFFFFFFF) for i in range(50)]
    u = SR.uniforms(0xDEADBEEF, -3, ids)
    assert (u.astype(np.float32).astype(np.float64) == u).all() and u.min() > 0 and u.max() < 1
    lo, hi = (0 + 0.5) * 2.0 ** -23, (2 ** 23 - 1 + 0.5) * 2.0 ** -23
    assert np.float32(lo) > 0 and np.float32(hi) < 1


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_sampling_refusals():
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    cfg = BertConfig.from_dict(json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json"))))
    ids = torch.zeros((1, 16), dtype=torch.int64)
    feat, loc = torch.zeros((1, 37, 192)), torch.zeros((1, 37, 5))
    model = BertForMultiModalPreTraining(cfg)
    with pytest.raises(ValueError, match="beams"):
        model.generate_answers(ids, feat, loc, [4], samples=2, beams=2)
    with pytest.raises(ValueError, match="samples"):
        model.generate_answers(ids, feat, loc, [4], samples=17)
    with pytest.raises(ValueError, match="temperature"):
        model.generate_answers(ids, feat, loc, [4], samples=2, temperature=0.0)
    with pytest.raises(ValueError, match="top_p"):
        model.generate_answers(ids, feat, loc, [4], samples=2, top_p=0.0)
    with pytest.raises(ValueError, match="top_k"):
        model.generate_answers(ids, feat, loc, [4], samples=2, top_k=-1)
    with pytest.raises(ValueError, match="streams"):
        model.generate_answers(ids, feat, loc, [4], samples=2, sample_streams=[0, 1])
    with pytest.raises(NotImplementedError):                        # the fp32x3 engine refuses as before
        BertForMultiModalPreTraining(cfg, compute_dtype="fp32x3").generate_answers(ids, feat, loc, [4], samples=2)
    assert GN.check_request([10, 250], 256, 1, 20, 1).tolist() == [20, 2]          # signature unchanged
    assert GN.SAMPLE_SITE == 0x30124877 and math.isfinite(GN.MAX_SAMPLES)


def test_entry_point_refuses_before_any_launch():
    """The argument checks of unimm_lm_sample return before anything touches a device: callable without a GPU (the pointers are
    never followed).  temperature <= 0 or not finite, top_p outside (0, 1], top_k < 0 and a missing pointer: UNIMM_E_ARG (-1); a
    bad shape: UNIMM_E_SHAPE (-2); rows = 0: OK."""
    from unimm_amd import build, lib
    build.build()
    f = lib.lib().unimm_lm_sample
    P = 4096                                                           # any non-NULL address

    def call(rows=0, V=30522, ldl=30522, t=1.0, k=0, p=1.0, streams=P, token=P, banned=0, nbanned=0):
        return f(P, rows, V, ldl, banned or None, nbanned, None, 102, t, k, p, 7, streams, token, P, P, None, None)

    assert call() == 0
    for kw in (dict(t=0.0), dict(t=-1.0), dict(t=float("nan")), dict(t=float("inf")), dict(p=0.0), dict(p=1.0001), dict(p=float("nan")),
               dict(k=-1), dict(streams=None), dict(token=None), dict(nbanned=3)):
        assert call(**kw) == -1, kw
    for kw in (dict(V=0), dict(V=65537, ldl=65537), dict(ldl=30521), dict(rows=-1), dict(nbanned=-1)):
        assert call(**kw) == -2, kw
    assert call(V=65536, ldl=65536, k=65536, p=1e-6) == 0
