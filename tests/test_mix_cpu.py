"""Ensemble and contrastive answer generation without a GPU: the reference of unimm_lm_mix (tests/mix_ref.py) against itself --
the float32 restatement against the float64 definition, the properties the header promises -- `beam_search` and `sample_search`
driven by a step function that mixes two table models, and every refusal of `generate_answers(ensemble=...)`."""
import copy
import inspect
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mix_ref as R
from tests import sample_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")
F32 = np.float32


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):                        # a row that is -inf throughout has no distribution (NaN)
        return x - R._lse64(x)[:, None]


# ---------------------------------------------------------------------------------------------------------------------------
# the reference against itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_logit_restatement_is_the_rounded_product_sum():
    """mix_f32 in LOGIT mode, element by element with numpy float32 scalars: every product and every sum rounded on its own.  It
    is NOT the float64 sum rounded once (what a fused multiply-add chain would approach) on some element of this input."""
    xs = R.edge_rows(16, 3, 5, 1, holes=False)
    w = R.logit_weights(5)
    got = R.mix_f32(xs, w, R.LOGIT, 16)
    for r, i in itertools.product(range(3), range(16)):
        z = F32(w[0]) * xs[0][r, i]
        for m in range(1, 5):
            z = F32(z + F32(F32(w[m]) * xs[m][r, i]))
        assert got[r, i].view(np.int32) == F32(z).view(np.int32)
    once = R.mix_f64(xs, w, R.LOGIT, 16).astype(F32)
    assert (once != got).any() and np.abs(once - got).max() < 1e-4


def test_prob_restatement_inside_budget():
    """PROB_BUDGET is the largest deviation of the float32 restatement from float64 over mix_ref.budget_cases(), rounded up."""
    worst, where = 0.0, None
    for name, V, K, xs, w in R.budget_cases():
        a, b = R.mix_f32(xs, w, R.PROB, V), R.mix_f64(xs, w, R.PROB, V)
        assert ((a == NEG) == (b == NEG)).all(), name
        fin = np.isfinite(b)
        d = float(np.abs(a[fin].astype(np.float64) - b[fin]).max()) if fin.any() else 0.0
        print(f"{name} K={K}: {d:.3e}")
        if d > worst:
            worst, where = d, (name, K)
    print(f"worst {worst:.4e} at {where}")
    assert 0.9 * R.PROB_BUDGET < worst <= R.PROB_BUDGET and where == ("wide", 5)


def test_one_member_is_the_member():
    x = R.edge_rows(257, 3, 2, 2, first=True)[1]
    fin = np.isfinite(x)
    assert (R.mix_f32([x], [1.0], R.LOGIT, 257)[fin].view(np.int32) == x[fin].view(np.int32)).all()
    got, want = R.mix_f64([x], [1.0], R.PROB, 257), log_softmax64(x)
    assert ((got == NEG) == ~fin).all() and np.abs(got[fin] - want[fin]).max() < 1e-12
    assert np.abs(R.mix_f32([x], [1.0], R.PROB, 257)[fin] - want[fin]).max() <= R.PROB_BUDGET


def test_identical_members_under_convex_weights_are_the_member():
    x = R.edge_rows(257, 3, 1, 3, holes=False)[0]
    for w in ([0.5, 0.5], [0.3, 0.7], [0.25, 0.0, 0.75], [0.2] * 5):
        got = R.mix_f64([x] * len(w), w, R.PROB, 257)
        assert np.abs(got - log_softmax64(x)).max() < 1e-6              # the weights are rounded to fp32: their sum is 1 +- 6e-8


def test_logit_weight_on_member_0_alone_returns_member_0():
    xs = R.edge_rows(257, 3, 4, 4, holes=False)
    got = R.mix_f32(xs, [1.0, 0.0, 0.0, 0.0], R.LOGIT, 257)
    assert (got == xs[0]).all()
    assert (R.mix_f32([xs[0], xs[0]], [0.5, 0.5], R.LOGIT, 257).view(np.int32) == xs[0].view(np.int32)).all()


def test_contrastive_score():
    """LOGIT (1, -1) with a cut is log p_expert - log p_amateur on the plausible ids, up to a constant per row"""
    V, sep = 257, 102
    xs = R.edge_rows(V, 4, 2, 5, holes=False)
    la = float(F32(np.log(0.1)))
    got = R.mix_f64(xs, [1.0, -1.0], R.LOGIT, V, None, None, sep, la)
    score = log_softmax64(xs[0]) - log_softmax64(xs[1])
    pe = log_softmax64(xs[0])
    for r in range(4):
        keep = np.isfinite(got[r])
        plausible = pe[r] >= pe[r].max() + np.log(0.1) - 1e-6
        assert (keep[plausible & (np.abs(pe[r] - pe[r].max() - np.log(0.1)) > 1e-5)]).all() and keep[sep]
        assert not keep[~plausible & (np.arange(V) != sep) & (np.abs(pe[r] - pe[r].max() - np.log(0.1)) > 1e-5)].any()
        c = got[r, keep] - score[r, keep]
        assert np.abs(c - c[0]).max() < 1e-9 and 1 < keep.sum() < V


def test_the_cut_keeps_sep_and_the_best_eligible_id():
    V, sep = 16, 5
    x = np.full((3, V), -40.0, dtype=F32)
    x[:, 3] = 1.0                                              # the best id ...
    x[1, 9] = 7.0                                              # ... but for row 1's banned 9 and row 2's flagged sep
    x[2, sep] = 7.0
    la = float(F32(np.log(0.5)))
    cut = R.cut_mask(x, [9], [0, 0, 1], sep, la)
    for r in range(3):
        assert sorted(np.nonzero(~cut[r])[0]) == sorted({3, sep} | ({9} if r == 1 else set())), r
    # a log_alpha above 0 cannot come from the generator, yet the best eligible id stays
    cut = R.cut_mask(x, [9], [0, 0, 1], sep, 1.0)
    assert not cut[:, 3].any() and not cut[:, sep].any() and cut[0].sum() == V - 2
    # nothing eligible: no cut
    assert not R.cut_mask(x[:, :2], [0, 1], None, 1, la).any()
    # off
    assert not R.cut_mask(x, None, None, sep, NEG).any()


def test_the_threshold_at_equality():
    """x_0,i < m0 + log_alpha in fp32: an id exactly at the threshold stays, the float below it goes"""
    V, sep = 16, 15
    for alpha in (0.1, 0.5, float(np.nextafter(F32(1), F32(0)))):
        la = F32(np.log(np.float64(alpha)))
        x = np.full((1, V), -50.0, dtype=F32)
        x[0, 2] = 3.25
        thr = F32(3.25) + la
        x[0, 4], x[0, 5], x[0, 6] = thr, np.nextafter(thr, F32(NEG)), min(np.nextafter(thr, F32(np.inf)), F32(3.25))
        cut = R.cut_mask(x, None, None, sep, float(la))
        assert not cut[0, 4] and cut[0, 5] and not cut[0, 6] and not cut[0, 2]
        for mode, w in ((R.LOGIT, [1.5, -0.5]), (R.PROB, [0.5, 0.5])):
            z = R.mix_f32([x, x[:, ::-1].copy()], w, mode, V, None, None, sep, float(la))
            assert ((z == NEG) == cut).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the searches on a mixture of two table models
# ---------------------------------------------------------------------------------------------------------------------------
SEP = SR.SEP
IDS = np.array([1, 2, 3, 4, SEP])                                  # the vocabulary of 5: four ids and [SEP]
SYM = {int(t): n for n, t in enumerate(IDS)}
LIMIT = 2                                                          # answers of up to 3 tokens, the [SEP] included
ALL = 1 + 4 + 16                                                   # the answers there are


def tables(seed, holes):
    """Two table models: log P_m[k, previous symbol] over the 5 symbols; holes (PROB only: a LOGIT mixture takes finite logits):
    one symbol of model 1 is impossible"""
    rng = np.random.RandomState(seed)
    out = []
    for m in range(2):
        p = rng.dirichlet(np.ones(5) * 0.8, size=(LIMIT + 1, 5))
        if m == 1 and holes:
            p[..., 2] = 0.0
            p /= p.sum(-1, keepdims=True)
        with np.errstate(divide="ignore"):
            out.append(np.log(p))
    return out


def mixture_rows(T, k, prev, weights, mode, flags):
    """log p of the 5 symbols for rows standing at step k after symbol prev[r], under the step rules (-inf where ruled out; no
    renormalisation)"""
    xs = [t[min(k, LIMIT), prev].astype(F32) for t in T]
    z = R.mix_f64(xs, weights, mode, 5, None, flags, 4, NEG)
    lp = z - R._lse64(z)[:, None]
    f = np.asarray(flags)
    lp[(f & 1) != 0, 4] = NEG
    lp[(f & 2) != 0, :4] = NEG
    return lp


def enumerate_answers(T, weights, mode, limit, drawn=False):
    """{answer: its summed log p under the mixture}; drawn: under the distribution a sampler draws from, every step renormalised
    over the ids the rules leave"""
    out = {}

    def walk(prefix, lp, k):
        row = mixture_rows(T, k, np.array([SYM[prefix[-1]] if prefix else 0]), weights, mode, [2 if k >= limit else 0])[0]
        if drawn:
            row = row - R._lse64(row[None])[0]
        for s in range(5):
            if row[s] > NEG:
                if s == 4:
                    out[prefix + (SEP,)] = lp + row[s]
                else:
                    walk(prefix + (int(IDS[s]),), lp + row[s], k + 1)
    walk((), 0.0, 0)
    return out


MIXES = (("prob", R.PROB, [0.6, 0.4]), ("logit", R.LOGIT, [0.7, 0.3]), ("contrast", R.LOGIT, [1.5, -0.5]))


@pytest.mark.parametrize("name,mode,weights", MIXES, ids=[m[0] for m in MIXES])
def test_full_width_beams_are_the_exhaustive_search_under_the_mixture(name, mode, weights):
    """beams = 21 holds every answer of up to 3 tokens over the 5-symbol vocabulary: the search is exhaustive, its best answer is
    the enumerated argmax under the mixture and every answer's summed step_logp its enumerated log-probability."""
    from unimm_amd.generation import beam_search
    G, B = 2, ALL
    Ts = [tables(11, mode == R.PROB), tables(12, mode == R.PROB)]
    limits = [LIMIT, 1]

    def step(k, parent, token, flags):
        vals = torch.full((G * B, B), NEG)
        ids = torch.zeros((G * B, B), dtype=torch.int64)
        for g in range(G):
            sl = slice(g * B, (g + 1) * B)
            prev = np.array([SYM.get(int(t), 0) for t in token[sl]]) if k else np.zeros(B, dtype=np.int64)
            lp = mixture_rows(Ts[g], k, prev, weights, mode, flags[sl].numpy())
            order = np.argsort(-lp, axis=1, kind="stable")
            vals[sl, :5] = torch.from_numpy(np.take_along_axis(lp, order, 1)).float()
            ids[sl, :5] = torch.from_numpy(IDS[order])
        return vals, ids

    got = beam_search(step, G, B, limits, LIMIT, min_answer_len=0)
    for g in range(G):
        want = enumerate_answers(Ts[g], weights, mode, limits[g])
        assert len(want) == (ALL if limits[g] == LIMIT else 5)
        best = max(want, key=lambda a: want[a])
        n = int(got.lengths[g, 0])
        assert tuple(got.tokens[g, 0, :n].tolist()) == best
        seen = set()
        for j in range(B):
            n = int(got.lengths[g, j])
            if n == 0:
                continue
            ans = tuple(got.tokens[g, j, :n].tolist())
            seen.add(ans)
            assert abs(float(got.step_logp[g, j, :n].sum()) - want[ans]) < 1e-5
            assert abs(float(got.logp[g, j]) - want[ans]) < 1e-5
        assert seen == set(want)


STREAMS = 16384


@pytest.mark.parametrize("name,mode,weights", MIXES[:2], ids=[m[0] for m in MIXES[:2]])
def test_sampling_draws_from_the_mixture(name, mode, weights):
    """16,384 streams through `sample_search`, each step an inverse-CDF draw from the float64 mixture row with a fixed generator:
    the joint distribution of whole answers against the enumerated mixture, chi^2 with cells of expected count < 5 pooled.  Fixed
    seeds, so deterministic: prob 20.48 (df 20, 0.1 % critical value 45.44), logit 21.90 (df 20, the same critical value); the summed step_logp of an
    answer is its enumerated log p under the mixture, the summed step_logq that under the renormalised rows drawn from."""
    from unimm_amd.generation import sample_search
    S = STREAMS
    T = tables(13, mode == R.PROB)
    rng = np.random.RandomState(5)

    def step(k, token, flags):
        prev = np.array([SYM.get(int(t), 0) for t in token.tolist()]) if k else np.zeros(S, dtype=np.int64)
        lp = mixture_rows(T, k, prev, weights, mode, flags.numpy())
        cdf = np.cumsum(np.exp(lp), 1)
        u = rng.random_sample(S) * cdf[:, -1]
        sym = np.minimum((u[:, None] >= cdf).sum(1), 4)
        lq = lp - R._lse64(lp)[:, None]
        return torch.from_numpy(IDS[sym]), torch.from_numpy(lp[np.arange(S), sym]).float(), torch.from_numpy(lq[np.arange(S), sym]).float()

    got = sample_search(step, S, 1, [LIMIT] * S, LIMIT, min_answer_len=0)
    want, raw = enumerate_answers(T, weights, mode, LIMIT, drawn=True), enumerate_answers(T, weights, mode, LIMIT)
    assert abs(sum(math.exp(v) for v in want.values()) - 1.0) < 1e-9
    counts = {}
    for row, n in zip(got.tokens[:, 0].tolist(), got.lengths[:, 0].tolist()):
        counts[tuple(row[:n])] = counts.get(tuple(row[:n]), 0) + 1
    assert set(counts) <= set(want)
    obs = np.array([counts.get(k, 0) for k in want], dtype=np.float64)
    exp = np.exp(np.array(list(want.values()))) * S
    big = exp >= 5
    o, e = obs[big], exp[big]
    if (~big).any():
        o, e = np.append(o, obs[~big].sum()), np.append(e, exp[~big].sum())
    stat, df = float(((o - e) ** 2 / e).sum()), len(e) - 1
    print(f"\n{name}: chi^2 {stat:.2f}, df {df}, critical {SR.chi_square_critical(df):.2f}")
    assert stat < SR.chi_square_critical(df) and df >= 10
    for row, n, lp, lq in list(zip(got.tokens[:, 0].tolist(), got.lengths[:, 0].tolist(), got.step_logp[:, 0].tolist(),
                                   got.step_logq[:, 0].tolist()))[:200]:
        assert abs(sum(lp[:n]) - raw[tuple(row[:n])]) < 1e-5 and abs(sum(lq[:n]) - want[tuple(row[:n])]) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------
# the refused requests
# ---------------------------------------------------------------------------------------------------------------------------
def _make(dtype="bf16", **over):
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json")))
    cfg.update(over)
    return BertForMultiModalPreTraining(BertConfig.from_dict(cfg), compute_dtype=dtype)


@pytest.fixture(scope="module")
def w():
    from unimm_amd.policy import frozen_reference
    torch.manual_seed(0)
    model = _make().eval()
    G, T, Rg = 2, 32, 5
    args = (torch.randint(1000, (G, T)), torch.randn(G, Rg, 192), torch.rand(G, Rg, 5), [6, 9])
    return dict(model=model, partner=frozen_reference(model), other=frozen_reference(model), args=args)


def test_the_keywords_are_keyword_only_and_off_by_default(w):
    from unimm_amd import generation
    from unimm_amd.modeling import BertForMultiModalPreTraining, VisualDialogEncoder
    for fn in (generation.generate_answers, BertForMultiModalPreTraining.generate_answers, VisualDialogEncoder.generate_answers):
        p = inspect.signature(fn).parameters
        names = ["ensemble", "ensemble_weights", "ensemble_mode", "plausibility"]
        assert list(p)[-7:-3] == names and list(p)[-3:] == ["draft_accept", "draft", "draft_len"]   # the older keywords stay last
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names)
        assert (p["ensemble"].default, p["ensemble_weights"].default, p["ensemble_mode"].default, p["plausibility"].default) == \
            (None, None, "prob", 0.0)


REFUSALS = (
    ("draft", dict(draft="partner"), "ensemble with draft"),
    ("empty", dict(ensemble=[]), "1 to 4 partner"),
    ("five", dict(ensemble="five"), "1 to 4 partner"),
    ("bare", dict(ensemble="bare"), "sequence of 1 to 4"),
    ("self", dict(ensemble="self"), "the model itself"),
    ("engine", dict(ensemble="engine"), "the model itself"),
    ("twice", dict(ensemble="twice"), "an earlier member again"),
    ("shared", dict(ensemble="shared"), "an earlier member again"),
    ("class", dict(ensemble=[torch.nn.Linear(2, 2)]), "BertForMultiModalPreTraining or a VisualDialogEncoder"),
    ("device", dict(ensemble="meta"), "move it with"),
    ("fp32x3", dict(ensemble="fp32x3"), "bf16 engine"),
    ("coatt", dict(ensemble="nocoatt"), "connection layers"),
    ("head", dict(ensemble="head"), "head size 32"),
    ("vocab", dict(ensemble=dict(vocab_size=1064)), "vocab_size"),
    ("feat", dict(ensemble=dict(v_feature_size=128)), "v_feature_size"),
    ("types", dict(ensemble=dict(type_vocab_size=3)), "type_vocab_size"),
    ("pos", dict(ensemble=dict(max_position_embeddings=256)), "max_position_embeddings"),
    ("count", dict(ensemble_weights=[1.0]), "1 ensemble_weights for 2 members"),
    ("count3", dict(ensemble_weights=[0.2, 0.3, 0.5]), "3 ensemble_weights for 2 members"),
    ("nan", dict(ensemble_weights=[0.5, float("nan")], ensemble_mode="logit"), "finite"),
    ("inf", dict(ensemble_weights=[0.5, float("inf")], ensemble_mode="logit"), "finite"),
    ("w0", dict(ensemble_weights=[0.0, 1.0]), "must be > 0"),
    ("w0logit", dict(ensemble_weights=[-1.0, 2.0], ensemble_mode="logit"), "must be > 0"),
    ("negative", dict(ensemble_weights=[1.5, -0.5]), "sum to 1"),
    ("sum", dict(ensemble_weights=[0.5, 0.6]), "sum to 1"),
    ("mode", dict(ensemble_mode="mean"), "ensemble_mode must be one of"),
    ("alpha1", dict(plausibility=1.0), r"plausibility must be in \[0, 1\)"),
    ("alpha-", dict(plausibility=-0.1), r"plausibility must be in \[0, 1\)"),
    ("alphanan", dict(plausibility=float("nan")), r"plausibility must be in \[0, 1\)"),
    ("cut+ngram", dict(plausibility=0.1, no_repeat_ngram_size=2), "could empty the plausible set"),
    ("cut+penalty", dict(plausibility=0.1, repetition_penalty=1.2), "could empty the plausible set"),
    ("weights alone", dict(ensemble=None, ensemble_weights=[1.0]), "need partner models"),
    ("cut alone", dict(ensemble=None, plausibility=0.1), "need partner models"),
)


@pytest.mark.parametrize("name,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_before_anything_is_staged(w, monkeypatch, name, kw, msg):
    from unimm_amd import lib as L
    from unimm_amd.engine import Engine

    def never(*a, **k):
        raise AssertionError("a refused request reached the engine")
    monkeypatch.setattr(L, "_call", never)
    monkeypatch.setattr(L, "lib", never)
    monkeypatch.setattr(Engine, "ensure", never)
    monkeypatch.setattr(Engine, "stage_host_inputs", never)
    kw = dict(kw)
    if kw.get("draft") == "partner":
        kw["draft"] = w["other"]
    e = kw.pop("ensemble", "partner")
    if e == "partner":
        e = [w["partner"]]
    elif e == "five":
        e = [copy.copy(w["partner"]) for _ in range(5)]
    elif e == "bare":
        e = w["partner"]
    elif e == "self":
        e = [w["model"]]
    elif e == "engine":
        d = copy.copy(w["partner"])
        d._engine = w["model"]._engine
        e = [d]
    elif e == "twice":
        e = [w["partner"], w["partner"]]
    elif e == "shared":
        d = copy.copy(w["other"])
        d._engine = w["partner"]._engine
        e = [w["partner"], d]
    elif e == "meta":
        e = [copy.deepcopy(w["partner"]).to("meta")]
    elif e == "fp32x3":
        e = [_make("fp32x3")]
    elif e == "nocoatt":
        d = copy.deepcopy(w["partner"])
        d.config = copy.copy(d.config)
        d.config.with_coattention = False
        e = [d]
    elif e == "head":
        e = [_make(num_attention_heads=4)]
    elif isinstance(e, dict):
        e = [_make(**e)]
    with pytest.raises(ValueError, match=msg):
        w["model"].generate_answers(*w["args"], ensemble=e, **kw)


def test_a_partner_of_another_depth_and_width_is_admitted(w):
    """depth, widths, head counts and the connection schedule are the partner's own: the checks pass, and the call goes on to the
    engine (which refuses a CPU model).  A VisualDialogEncoder-shaped wrapper is unwrapped."""
    from unimm_amd import lib as L
    from unimm_amd.generation import check_ensemble, check_partner
    d = _make(num_hidden_layers=2, v_num_hidden_layers=1, t_biattention_id=[1], v_biattention_id=[0], hidden_size=64,
              num_attention_heads=1, intermediate_size=128)
    assert check_partner(w["model"], d, 1) is d

    class Wrapped:
        bert_pretrained = d
    e = check_ensemble(w["model"], [Wrapped(), w["partner"]], None, "prob", 0.0)
    assert e["partners"] == [d, w["partner"]] and e["weights"] == [1 / 3] * 3 and e["log_alpha"] == NEG and e["mode"] == "prob"
    e = check_ensemble(w["model"], (d,), np.array([1.5, -0.5]), "logit", 0.1)
    assert e["weights"] == [1.5, -0.5] and e["log_alpha"] == float(np.float32(np.log(0.1)))
    assert check_ensemble(w["model"], None) is None
    with pytest.raises(L.UnimmHipError):
        w["model"].generate_answers(*w["args"], ensemble=[d])
