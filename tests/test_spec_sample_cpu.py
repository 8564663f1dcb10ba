"""Speculative sampling without a GPU: the reference of unimm_lm_spec_verify (tests/spec_sample_ref.py) against its own float32
restatement and its cap on undecided rows, the rejection rule's exactness on a table model through `speculative_sample_search`,
the greedy rows against `speculative_search` / `beam_search`, the step-keyed streams, and the refusals of
generate_answers(draft_accept=...) before anything is staged."""
import inspect
import math

import numpy as np
import pytest
import torch

from tests import sample_ref as SR
from tests import spec_sample_ref as R


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
def f32_outputs(V, no):
    """The float32 restatement of launch `no` of spec_case(V) as if it were the kernel's outputs."""
    rp, rq = R.case_rows(V)
    t, k, p = R.launch_params(V, no)
    d = R.drafts(V, no)
    n = len(rp)
    out = dict(accept=np.zeros(n, np.int32), token=np.full(n, -1, np.int32), logp=np.full(n, -np.inf, np.float32),
               logq=np.full(n, -np.inf, np.float32), lse=np.zeros(n, np.float32), log_ratio=np.full(n, -np.inf, np.float32))
    for r in range(n):
        out["lse"][r] = rp[r].lse
        r32 = R.verify_row_f32(rp[r], rq[r], int(d[r]), t[r], int(k[r]), p[r], R.KEY_ACCEPT, V)
        if r32 is None:
            continue
        tk = r32["token"]
        out["accept"][r], out["token"][r], out["logq"][r], out["log_ratio"][r] = r32["accept"], tk, r32["logq"], r32["a"]
        out["logp"][r] = np.float32(rp[r].xall[tk]) - np.float32(rp[r].lse)
    return out, d, (t, k, p)


@pytest.mark.parametrize("V", R.SPEC_V)
def test_f32_restatement_inside_budgets(V):
    """The float32 restatement satisfies the checker of the GPU suite, its ratios are 8 x inside the constants, and the
    reference alone leaves at most 2 % of the non-planted rows undecided (the cap the GPU suite asserts)."""
    rp, rq = R.case_rows(V)
    names = R.spec_case(V)["names"]
    plain = np.nonzero([nm.startswith("random") for nm in names])[0]
    wa = wr = 0.0
    draws = undecided = 0
    for no in range(R.LAUNCHES):
        out, d, params = f32_outputs(V, no)
        R.check_launch(rp, rq, d, params, R.KEY_ACCEPT, V, out, what=f"V {V} launch {no}")
        n, u = R.check_launch([rp[r] for r in plain], [rq[r] for r in plain], d[plain], tuple(a[plain] for a in params), R.KEY_ACCEPT,
                              V, {k: v[plain] for k, v in out.items()})
        draws, undecided = draws + n, undecided + u
        for r in range(len(rp)):
            a, b = R.measure_row(rp[r], rq[r], int(d[r]), params[0][r], int(params[1][r]), params[2][r], R.KEY_ACCEPT, V)
            wa, wr = max(wa, a), max(wr, b)
    print(f"\nV = {V}: accept ratio {wa:.3f} (C_ACC {R.C_ACC}), residual ratio {wr:.3f} (C_RES {R.C_RES}); "
          f"{undecided} of {draws} non-planted rows undecided")
    assert 8 * wa <= R.C_ACC and 8 * wr <= R.C_RES
    assert draws > 60 and undecided <= R.UNDECIDED_CAP * draws


def test_constants_are_the_measured_ones():
    assert R.C_ACC == SR.pow2_at_least(8 * R.ACC_MEASURED) and R.C_RES == SR.pow2_at_least(8 * R.RES_MEASURED)


def test_planted_rows_are_what_they_say():
    for V in (16, 257):
        c = R.spec_case(V)
        rp, rq = R.case_rows(V)
        pl = c["plant"]
        assert set(pl) == set(R.PLANTED)
        assert torch.equal(c["x"][pl["xd equal to x"]], c["xd"][pl["xd equal to x"]])
        r = pl["disjoint supports"]
        assert rp[r].n > 0 and rq[r].n > 0 and not set(rp[r].ids) & set(rq[r].ids)
        assert rq[pl["xd all -inf"]].n == 0 and rp[pl["xd all -inf"]].n > 0
        r = pl["P <= Q on all ids but one"]
        rd = R.verify_row(rp[r], rq[r], int(rp[r].ids[0]), 1.0, 0, 1.0, R.KEY_ACCEPT, V)[0]
        assert rd["allowed"] == {int(rp[r].ids[1])} and rd["res_decided"]
        for no in range(R.LAUNCHES):
            d = R.drafts(V, no)
            assert d[pl["no draft"]] == -1 and d[pl["d >= V"]] >= V and d[pl["d = -2"]] == -2


def test_mirror_meets_both_distributions():
    """The float64 mirror of the whole rule over the 65,536 streams and the keys of the device's distribution test: chi^2 of the
    cells (accept, token) against n min(P~, Q~) / n max(0, P~ - Q~) = 18.66 with 21 degrees of freedom (critical 46.8)."""
    x, xd = R.pair16()
    acc, tok, d = R.mirror_streams(x, xd, 0.7, np.arange(65536))
    P, Q = R.softmax_kept(x, 0.7), R.softmax_kept(xd, 0.7)
    stat, df = R.chi_square_cells(acc, tok, P, Q)
    print(f"\nmirror: chi^2 {stat:.2f}, df {df}, critical {SR.chi_square_critical(df):.2f}, acceptance {acc.mean():.4f} "
          f"(sum min(P, Q) = {np.minimum(P, Q).sum():.4f})")
    assert stat < SR.chi_square_critical(df) and df >= 15
    assert abs(acc.mean() - np.minimum(P, Q).sum()) < 4 * math.sqrt(0.25 / 65536)


# ---------------------------------------------------------------------------------------------------------------------------
# the loop on table models
# ---------------------------------------------------------------------------------------------------------------------------
SEP = SR.SEP
IDS = np.array([0, 1, 2, 3, 4, 5, 6, SEP])                          # the vocabulary of 8: seven ids and [SEP]
SYM = {int(t): n for n, t in enumerate(IDS)}
SEED, LIMIT = 11, 2                                                 # at most two tokens and the forced [SEP]: answers of <= 3


def tables(kind):
    """(P, Q) [step, previous symbol, symbol] of a Markov table model; Q by `kind`: equal to P, disjoint in support (P on the
    even symbols and [SEP], Q on the odd ones), or overlapping (another draw, with two of P's symbols missing)."""
    rng = np.random.default_rng(5)
    P = rng.random((LIMIT + 1, 8, 8)) + 0.05
    P[..., 7] *= 0.6
    Q = rng.random((LIMIT + 1, 8, 8)) + 0.05
    if kind == "equal":
        Q = P.copy()
    elif kind == "disjoint":
        P[..., 1:7:2] = 0.0
        Q[..., 0:7:2] = 0.0
        Q[..., 7] = 0.0
    else:
        Q[..., [2, 5]] = 0.0
        P[..., 3] = 0.0
    return P / P.sum(-1, keepdims=True), Q / Q.sum(-1, keepdims=True)


def ruled(p, flags):
    """The step rules on rows of probabilities [S, 8]: [SEP] banned / forced, renormalised (the filtered distribution)."""
    p = p.copy()
    f = np.asarray(flags)
    p[(f & 1) != 0, 7] = 0.0
    forced = (f & 2) != 0
    p[forced, :7] = 0.0
    p[forced, 7] = 1.0
    return p / p.sum(-1, keepdims=True)


def noise(site, k, streams):
    """u [S, 8] of (dropout.make_key(SEED, k[s], site), streams[s], id): the sampler's uniforms, keyed by the ABSOLUTE step."""
    from unimm_amd import dropout as DR
    keys = np.array([DR.make_key(SEED, int(a), site) for a in range(int(np.max(k)) + 1)], dtype=np.uint64)[np.asarray(k)]
    f = (np.asarray(streams).astype(np.uint64) * np.uint64(0x9E3779B1) + np.uint64(0x7F4A7C15)) & SR.M32
    sk = SR.mix32_np(keys ^ f)
    h = SR.mix32_np(sk[:, None] + ((IDS.astype(np.uint64) * np.uint64(0x85EBCA77)) & SR.M32)[None])
    return ((h >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel_argmax(p, u):
    with np.errstate(divide="ignore"):
        return np.argmax(np.where(p > 0, np.log(p), -np.inf) - np.log(-np.log(u)), 1)


def mirror_steps(P, Q, S, g, greedy_rows=None):
    """SpecSampleSteps of the float64 mirror of the kernels over S slots (stream = slot); greedy_rows: slots that keep one id."""
    from unimm_amd import speculative as SP
    streams = np.arange(S)
    sym = np.vectorize(SYM.get)
    rows = np.arange(S)

    def dist(T, k, prev, flags):
        p = ruled(T[np.minimum(k, LIMIT), prev], flags)
        if greedy_rows is not None:                                  # top_k = 1: the first id of the rank order
            top = np.zeros_like(p)
            top[rows, np.argmax(p, 1)] = 1.0
            p = np.where(greedy_rows[:, None], top, p)
        return p

    def root(flags):
        p = dist(P, np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64), flags.numpy())
        t = gumbel_argmax(p, noise(SP.RESIDUAL_SITE, np.zeros(S, dtype=np.int64), streams))
        lp = np.log(p[rows, t])
        return torch.from_numpy(lp).float(), torch.from_numpy(lp).float(), torch.from_numpy(IDS[t])

    def draft(j, n, token, flags, hist):
        k = n.numpy() + j
        q = dist(Q, k, sym(token.numpy()), flags.numpy())
        return torch.from_numpy(IDS[gumbel_argmax(q, noise(SP.DRAFT_SITE, k, streams))])

    def verify(n, last, drafts, flags, hist):
        out = [np.zeros((S, g + 1)) for _ in range(4)]
        for j in range(g + 1):
            k = n.numpy() + j
            prev = sym((last if j == 0 else drafts[:, j - 1]).numpy())
            p = dist(P, k, prev, flags[:, j].numpy())
            if j < g:
                q = dist(Q, k, prev, flags[:, j].numpy())
                d = sym(drafts[:, j].numpy())
                with np.errstate(divide="ignore"):
                    a = np.log(p[rows, d]) - np.log(q[rows, d])
                acc = np.log(noise(SP.ACCEPT_SITE, k, streams)[:, 0]) < a
                res = np.maximum(p - q, 0.0)
                res = np.where(res.sum(1, keepdims=True) > 0, res, p)
            else:
                d, acc, res = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=bool), p
            t = np.where(acc, d, gumbel_argmax(res, noise(SP.RESIDUAL_SITE, k, streams)))
            out[0][:, j] = out[1][:, j] = np.log(p[rows, t])
            out[2][:, j], out[3][:, j] = IDS[t], acc
        return (torch.from_numpy(out[0]).float(), torch.from_numpy(out[1]).float(), torch.from_numpy(out[2]).long(),
                torch.from_numpy(out[3]).long())

    return SP.SpecSampleSteps(root, draft, verify, lambda n, emit, live: None)


def sequence_probabilities(P):
    """{answer tuple: probability} under the model alone with the step rules (min_answer_len = 0, [SEP] forced at LIMIT)."""
    out = {}

    def walk(prefix, prob, k):
        flags = np.array([2 if k >= LIMIT else 0])
        p = ruled(P[min(k, LIMIT), SYM[prefix[-1]] if prefix else 0][None], flags)[0]
        for s in range(8):
            if p[s] > 0:
                if s == 7:
                    out[prefix + (SEP,)] = prob * p[s]
                else:
                    walk(prefix + (int(IDS[s]),), prob * p[s], k + 1)
    walk((), 1.0, 0)
    return out


EXACT = {"equal": (3, 24576), "disjoint": (2, 24576), "overlap": (1, 24576), "overlap3": (3, 24576)}


@pytest.mark.parametrize("case", list(EXACT))
def test_rejection_rule_is_exact_on_a_table_model(case):
    """24,576 streams through `speculative_sample_search` driven by the float64 mirror (noise keyed by the absolute step): the
    joint distribution of whole answers against the product of the model's own P~, chi^2 with cells of expected count < 5
    pooled.  Fixed keys, so deterministic: equal 39.67 (df 56), disjoint 13.18 (df 20), overlap 25.34 (df 42) with draft_len 1 and
    with draft_len 3 (the same figure only because LIMIT = 2 forces step 2 to [SEP] on both sides: in general another draft_len gives
    other draws of the same distribution -- test_a_seed_fixes_the_answers_for_a_given_draft_len); the 0.1 % critical values are
    94.5, 45.4 and 76.2."""
    from unimm_amd.speculative import speculative_sample_search
    g, S = EXACT[case]
    P, Q = tables(case.rstrip("3"))
    got = speculative_sample_search(mirror_steps(P, Q, S, g), S, 1, [LIMIT] * S, LIMIT, g, min_answer_len=0)
    want = sequence_probabilities(P)
    assert abs(sum(want.values()) - 1.0) < 1e-12
    counts = {}
    for row, n in zip(got.tokens[:, 0].tolist(), got.lengths[:, 0].tolist()):
        counts[tuple(row[:n])] = counts.get(tuple(row[:n]), 0) + 1
    assert set(counts) <= set(want)
    obs = np.array([counts.get(k, 0) for k in want], dtype=np.float64)
    exp = np.array(list(want.values())) * S
    big = exp >= 5
    o, e = obs[big], exp[big]
    if (~big).any():
        o, e = np.append(o, obs[~big].sum()), np.append(e, exp[~big].sum())
    stat, df = float(((o - e) ** 2 / e).sum()), len(e) - 1
    sp = got.speculation
    rate = int(sp.accepted.sum()) / int(sp.drafted.sum())
    print(f"\n{case}: chi^2 {stat:.2f}, df {df}, critical {SR.chi_square_critical(df):.2f}; acceptance {rate:.3f}, rounds {sp.rounds}")
    assert stat < SR.chi_square_critical(df) and df >= 10
    if case == "equal":
        assert (sp.per_round[sp.per_round >= 0] >= 1).all() and rate > 0.4        # Q~ = P~: log ratio 0, every draft accepted
    elif case == "disjoint":
        assert int(sp.accepted.max()) <= 1                           # only the [SEP] both models are forced to at the limit
    else:
        assert 0.0 < rate < 1.0
    # step_logp / step_logq are the emitted tokens' own log P~, whichever way they were emitted
    for row, n, lp in list(zip(got.tokens[:, 0].tolist(), got.lengths[:, 0].tolist(), got.step_logp[:, 0].tolist()))[:200]:
        assert abs(sum(lp[:n]) - math.log(want[tuple(row[:n])])) < 1e-4
    assert torch.equal(got.step_logp, got.step_logq) and sp.drafted.shape == (S, 1)


def test_a_seed_fixes_the_answers_for_a_given_draft_len():
    """Answers of up to 5 tokens, longer than draft_len + 1: the same seed and draft_len repeat the answers; another draft_len
    gives other draws (whether a step is a drafted row or the bonus row, a plain draw, depends on draft_len) of the same
    distribution -- the length histograms of 4,096 slots agree within sampling error."""
    from unimm_amd.speculative import speculative_sample_search
    S, lim = 4096, 5
    P, Q = tables("overlap")
    run = lambda g: speculative_sample_search(mirror_steps(P, Q, S, g), S, 1, [lim] * S, lim, g, min_answer_len=0)   # noqa: E731
    a, b, c = run(1), run(1), run(3)
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.step_logp, b.step_logp)
    same = int((a.tokens == c.tokens).all(-1).sum())
    assert int(a.lengths.max()) > 4 and 0 < same < S
    ha, hc = (torch.bincount(r.lengths[:, 0], minlength=lim + 2).double() for r in (a, c))
    assert ((ha - hc).abs() <= 5 * (ha + hc + 1).sqrt()).all(), (ha, hc)


def greedy_steps(G, B, banned, gamma, kind):
    """The table model of tests/test_speculative_cpu.py with top_k = 1 on both sides, as SpecSampleSteps over S = G * B slots
    (slot s decodes dialog s // B): the model's token with log q = 0, accept = (draft == token)."""
    import zlib
    from tests import test_speculative_cpu as TS
    from unimm_amd.speculative import SpecSampleSteps
    S = G * B
    state = {}

    def target(s, prefix, flags):
        return TS.top1(TS.ruled(TS.table_row(s // B, prefix), int(flags), banned))

    def root(flags):
        out = [target(s, [], flags[s]) for s in range(S)]
        v = torch.stack([o[0] for o in out])
        return v, torch.zeros_like(v), torch.tensor([o[1] for o in out])

    def draft(j, n, token, flags, hist):
        if j == 0:
            state["prefix"] = [hist[s, :int(n[s])].tolist() for s in range(S)]
        else:
            for s in range(S):
                state["prefix"][s].append(int(token[s]))
        out = []
        for s in range(S):
            p = state["prefix"][s]
            t = target(s, p, flags[s])[1]
            if kind == "wrong" or (kind == "random" and zlib.crc32(repr(("agree", s // B, len(p))).encode()) % 3 == 0):
                t = TS.other(t)
            elif kind == "early_sep" and len(p) >= 2:
                t = SEP
            out.append(t)
        return torch.tensor(out)

    def verify(n, last, drafts, flags, hist):
        vals, ids = torch.zeros(S, gamma + 1), torch.zeros(S, gamma + 1, dtype=torch.int64)
        for s in range(S):
            p = hist[s, :int(n[s])].tolist()
            for j in range(gamma + 1):
                vals[s, j], ids[s, j] = target(s, p + drafts[s, :j].tolist(), flags[s, j])
        acc = torch.cat([(drafts == ids[:, :gamma]).long(), torch.zeros(S, 1, dtype=torch.int64)], 1)
        return vals, torch.zeros_like(vals), ids, acc

    def commit(n, emit, live):
        assert (emit[~live] == 0).all() and (emit[live] >= 1).all() and (emit <= gamma + 1).all()

    return SpecSampleSteps(root, draft, verify, commit)


@pytest.mark.parametrize("kind,gamma", (("equal", 4), ("wrong", 2), ("random", 3), ("early_sep", 15)))
def test_greedy_rows_equal_the_greedy_searches(kind, gamma):
    """top_k = 1 on both sides: the rejection loop is `speculative_search` and `beam_search(beams=1)` -- tokens, lengths and
    step_logp exactly, the greedy slot's sums too; round counts, mixed limits and min_answer_len as in the greedy CPU tests."""
    from tests import test_speculative_cpu as TS
    from unimm_amd.speculative import speculative_sample_search
    for rule in range(len(TS.RULES)):
        limits, max_len, min_len, banned = TS.RULES[rule]
        G = len(limits)
        want = TS.plain_of(rule)
        ref = TS.speculative(G, limits, max_len, min_len, banned, gamma, kind)
        got = speculative_sample_search(greedy_steps(G, 2, banned, gamma, kind), G, 1, limits, max_len, gamma, min_len, greedy=True)
        for a in (got, got.greedy):
            assert torch.equal(a.tokens, want.tokens) and torch.equal(a.lengths, want.lengths)
            assert torch.equal(a.step_logp, want.step_logp)
        assert torch.equal(got.greedy.logp, want.logp) and torch.equal(got.greedy.scores, want.scores)
        assert torch.allclose(got.logp, want.logp, atol=1e-5) and float(got.step_logq.abs().max()) == 0.0
        assert got.speculation.rounds == ref.speculation.rounds == got.greedy.speculation.rounds
        assert torch.equal(got.speculation.accepted[:, 0], ref.speculation.accepted)
        assert torch.equal(got.speculation.drafted[:, 0], ref.speculation.drafted)
        assert torch.equal(got.greedy.speculation.per_round, ref.speculation.per_round)
        assert got.speculation.per_round.shape == (ref.speculation.rounds, G, 1)
        assert (got.lengths[:, 0] <= torch.tensor(limits) + 1).all()
        L = want.lengths[:, 0]
        if kind == "equal":
            assert got.speculation.rounds == int(torch.ceil((L - 1) / (gamma + 1)).max())
        if kind == "wrong":
            assert got.speculation.rounds == int(L.max()) - 1 and int(got.speculation.accepted.sum()) == 0


def test_step_streams_key_rows_by_their_own_step():
    """A launch keyed by site_key alone with step_streams' ids hashes as a launch keyed by make_key(seed, k, site) does."""
    from unimm_amd import dropout as DR
    from unimm_amd import speculative as SP
    salts = torch.tensor([DR.step_salt(SEED, k) for k in range(40)], dtype=torch.int64)
    st = torch.tensor([0, 1, -5, 2 ** 31 - 1, -2 ** 31, 77, 123456789], dtype=torch.int32)
    assert len({SP.DRAFT_SITE, SP.ACCEPT_SITE, SP.RESIDUAL_SITE}) == 3
    for k in (0, 1, 7, 39):
        moved = SP.step_streams(st, torch.full((len(st),), k), salts)
        assert moved.dtype == torch.int32
        for site in (SP.DRAFT_SITE, SP.ACCEPT_SITE, SP.RESIDUAL_SITE):
            for a, b in zip(st.tolist(), moved.tolist()):
                assert SR.stream_key(DR.make_key(SEED, k, site), a) == SR.stream_key(DR.site_key(SEED, site), b)


# ---------------------------------------------------------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def w():
    from tests import test_speculative_cpu as TS
    from unimm_amd.policy import frozen_reference
    torch.manual_seed(0)
    model = TS._make().eval()
    G, T, R = 2, 32, 5
    args = (torch.randint(1000, (G, T)), torch.randn(G, R, 192), torch.rand(G, R, 5), [6, 9])
    return dict(model=model, draft=frozen_reference(model), args=args)


NEW_REFUSALS = (
    ("no samples", dict(draft_accept="rejection"), "needs samples >= 1"),
    ("no draft", dict(draft_accept="rejection", samples=2, draft=None), "needs a draft"),
    ("word", dict(draft_accept="reject", samples=2), "draft_accept must be"),
    ("default refuses samples", dict(samples=2), "speculative sampling"),
    ("match refuses samples", dict(draft_accept="match", samples=2), "draft_accept='rejection'"),
    ("beams", dict(draft_accept="rejection", samples=2, beams=2), "draws independent answers and needs beams = 1"),
    ("ngram", dict(draft_accept="rejection", samples=2, no_repeat_ngram_size=2), "history rules"),
    ("penalty", dict(draft_accept="rejection", samples=2, repetition_penalty=1.3), "history rules"),
    ("scope", dict(draft_accept="rejection", samples=2, repeat_scope="dialog"), "history rules"),
    ("len16", dict(draft_accept="rejection", samples=2, draft_len=16), "draft_len"),
    ("self", dict(draft_accept="rejection", samples=2, draft="self"), "the model itself"),
    ("samples 17", dict(draft_accept="rejection", samples=17), "samples must be"),
    ("greedy 16", dict(draft_accept="rejection", samples=16, greedy=True), "slots exceed"),
    ("temperature", dict(draft_accept="rejection", samples=2, temperature=0.0), "temperature"),
)


@pytest.mark.parametrize("name,kw,msg", NEW_REFUSALS, ids=[r[0] for r in NEW_REFUSALS])
def test_new_refusals_before_anything_is_staged(w, monkeypatch, name, kw, msg):
    from unimm_amd import lib as L
    from unimm_amd.engine import Engine

    def never(*a, **k):
        raise AssertionError("a refused request reached the engine")
    for obj, attr in ((L, "_call"), (L, "lib"), (Engine, "ensure"), (Engine, "stage_host_inputs")):
        monkeypatch.setattr(obj, attr, never)
    kw = dict(kw)
    d = kw.pop("draft", w["draft"])
    d = w["model"] if d == "self" else d
    with pytest.raises(ValueError, match=msg):
        w["model"].generate_answers(*w["args"], draft=d, **kw)


def test_the_keyword_is_keyword_only_and_off_by_default(w):
    from unimm_amd import generation, trainer
    from unimm_amd.modeling import BertForMultiModalPreTraining, VisualDialogEncoder
    for fn in (generation.generate_answers, BertForMultiModalPreTraining.generate_answers, VisualDialogEncoder.generate_answers):
        p = inspect.signature(fn).parameters
        assert list(p)[-3:] == ["draft_accept", "draft", "draft_len"]
        assert p["draft_accept"].default == "match" and p["draft_accept"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(trainer.self_critical_step).parameters
    assert p["draft"].default is None and p["draft_len"].default == 4
    assert p["draft"].kind is p["draft_len"].kind is inspect.Parameter.KEYWORD_ONLY


def test_an_admitted_request_goes_on_to_the_engine(w):
    """samples with draft_accept='rejection' (and a greedy slot) pass every host check: the engine then refuses the CPU model"""
    from unimm_amd import lib as L
    with pytest.raises(L.UnimmHipError):
        w["model"].generate_answers(*w["args"], draft=w["draft"], draft_accept="rejection", samples=3, greedy=True, top_k=[0, 5, 1],
                                    draft_len=15)
