"""Speculative greedy answer generation without a GPU: `speculative_search` driven by table models against
`beam_search(beams=1)`, the pair rule of unimm_attn_verify against the generative mask, the fp32 restatement of the kernel inside
its budget, and the refused requests."""
import json
import math
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import generate_ref as GR
from oracle import masks
from tests import spec_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEP, V = 102, 160
NEG = float("-inf")


# ---------------------------------------------------------------------------------------------------------------------------
# table models
# ---------------------------------------------------------------------------------------------------------------------------
def table_row(g, prefix, salt=0):
    """fp32 log-softmax row of dialog g after `prefix`: a function of (g, prefix) only; [SEP] gains with the length."""
    seed = zlib.crc32(repr((salt, g, tuple(int(t) for t in prefix))).encode())
    x = torch.randn(V, generator=torch.Generator().manual_seed(seed)) * 2
    x[SEP] += 0.9 * len(prefix) - 2.5
    return torch.log_softmax(x.float(), 0)


def ruled(row, flags, banned):
    row = row.clone()
    row[list(banned)] = NEG
    if flags & 1:
        row[SEP] = NEG
    if flags & 2:
        keep = row[SEP].clone()
        row[:] = NEG
        row[SEP] = keep
    return row


def top1(row):
    i = int(np.lexsort((np.arange(V), -row.numpy()))[0])               # value desc, id asc
    return row[i], i


def plain(G, limits, max_len, min_len, banned):
    """beam_search(beams = 1) on the table model."""
    from unimm_amd.generation import beam_search
    prefix = [[] for _ in range(G)]

    def step(k, parent, token, flags):
        vals, ids = torch.zeros(G, 1), torch.zeros(G, 1, dtype=torch.int64)
        for g in range(G):
            if k > 0:
                prefix[g].append(int(token[g]))
            vals[g, 0], ids[g, 0] = top1(ruled(table_row(g, prefix[g]), int(flags[g]), banned))
        return vals, ids

    return beam_search(step, G, 1, limits, max_len, min_len)


def other(t):
    return 7 if t != 7 else 8


DRAFTS = ("equal", "wrong", "random", "early_sep")


def speculative(G, limits, max_len, min_len, banned, gamma, kind, log=None):
    from unimm_amd.speculative import SpecSteps, speculative_search
    state = dict(prefix=None)

    def target(g, prefix, flags):
        return top1(ruled(table_row(g, prefix), int(flags), banned))

    def root(flags):
        out = [target(g, [], flags[g]) for g in range(G)]
        return torch.stack([o[0] for o in out]), torch.tensor([o[1] for o in out])

    def draft(j, n, token, flags, hist):
        if j == 0:
            state["prefix"] = [hist[g, :int(n[g])].tolist() for g in range(G)]
            for g in range(G):
                assert state["prefix"][g][-1] == int(token[g])
        else:
            for g in range(G):
                state["prefix"][g].append(int(token[g]))
        out = []
        for g in range(G):
            p = state["prefix"][g]
            t = target(g, p, flags[g])[1]
            if kind == "wrong":
                t = other(t)
            elif kind == "random" and zlib.crc32(repr(("agree", g, len(p))).encode()) % 3 == 0:
                t = other(t)
            elif kind == "early_sep" and len(p) >= 2:
                t = SEP
            out.append(t)
        return torch.tensor(out)

    def verify(n, last, drafts, flags, hist):
        vals, ids = torch.zeros(G, gamma + 1), torch.zeros(G, gamma + 1, dtype=torch.int64)
        for g in range(G):
            p = hist[g, :int(n[g])].tolist()
            assert p[-1] == int(last[g])
            for j in range(gamma + 1):
                vals[g, j], ids[g, j] = target(g, p + drafts[g, :j].tolist(), flags[g, j])
        return vals, ids

    def commit(n, emit, live):
        assert (emit[~live] == 0).all() and (emit[live] >= 1).all() and (emit <= gamma + 1).all()
        if log is not None:
            log.append(emit.clone())

    return speculative_search(SpecSteps(root, draft, verify, commit), G, limits, max_len, gamma, min_len)


RULES = (  # (limits, max_answer_len, min_answer_len, banned)
    ([0, 1, 5, 12, 12], 12, 0, (0, 101, 103)),
    ([1, 3, 7, 12, 2], 12, 1, (0, 101, 103)),
    ([3, 4, 12, 9, 12], 12, 3, (0, 101, 103)),
    ([2, 12, 6, 12, 12], 12, 1, (5, 6, 7, 8, 101, 140)),
)
_plain = {}


def plain_of(rule):
    if rule not in _plain:
        limits, max_len, min_len, banned = RULES[rule]
        _plain[rule] = plain(len(limits), limits, max_len, min_len, banned)
    return _plain[rule]


@pytest.mark.parametrize("gamma", (1, 2, 4, 15))
@pytest.mark.parametrize("kind", DRAFTS)
@pytest.mark.parametrize("rule", range(len(RULES)))
def test_table_model_search_equals_beam_search(rule, kind, gamma):
    limits, max_len, min_len, banned = RULES[rule]
    G = len(limits)
    want = plain_of(rule)
    got = speculative(G, limits, max_len, min_len, banned, gamma, kind)
    assert torch.equal(got.tokens, want.tokens)
    assert torch.equal(got.lengths, want.lengths)
    assert torch.equal(got.step_logp, want.step_logp)
    assert torch.equal(got.logp, want.logp)
    assert torch.equal(got.scores, want.scores)
    assert (got.lengths[:, 0] <= torch.tensor(limits) + 1).all()
    sp = got.speculation
    L = want.lengths[:, 0]
    if kind == "equal":
        assert sp.rounds == int(torch.ceil((L - 1) / (gamma + 1)).max())
    if kind == "wrong":
        assert sp.rounds == int(L.max()) - 1
        assert int(sp.accepted.sum()) == 0
    # the counts add up: gamma drafts per live round; every live round emits its accepted drafts and one token of the model's
    # own, except that a round ending in an ACCEPTED [SEP] emits no token after it
    live_rounds = (sp.per_round >= 0).sum(0)
    assert sp.per_round.shape == (sp.rounds, G)
    assert torch.equal(sp.drafted, gamma * live_rounds)
    assert torch.equal(sp.accepted, sp.per_round.clamp_min(0).sum(0))
    own = L - 1 - sp.accepted
    assert ((own == live_rounds) | (own == live_rounds - 1)).all() and (sp.accepted <= sp.drafted).all()


def test_mixed_acceptance_in_one_round():
    """the random draft makes the dialogs of one batch advance at different rates"""
    limits, max_len, min_len, banned = RULES[3]
    log = []
    got = speculative(len(limits), limits, max_len, min_len, banned, 4, "random", log)
    pr = got.speculation.per_round
    assert any(len(set(r[r >= 0].tolist())) > 1 for r in pr)
    assert len(log) == got.speculation.rounds and 0 < int(got.speculation.accepted.sum()) < int(got.speculation.drafted.sum())


# ---------------------------------------------------------------------------------------------------------------------------
# the pair rule is the generative mask
# ---------------------------------------------------------------------------------------------------------------------------
def test_pair_rule_equals_the_generative_mask():
    """A completed sequence laid out by oracle/masks.py: for every round state (n tokens emitted, g drafts), the key set the
    pair rule gives new row i -- context [1, c), private answer rows [0, n - 1), the new rows pair_keys(i) -- is that row's row
    of the generative mask."""
    from unimm_amd.speculative import pair_keys
    assert all(pair_keys(i) == SR.pair_keys(i) for i in range(32))
    answer = [11, 12, 13, 14, 15, 16, 17, 18, 19]
    enc = masks.encode_gen([[5, 6, 7], [8, 9], answer], max_seq_len=64)
    m = np.asarray(enc["txt_attention_mask"][0]).astype(bool)
    A = len(answer) + 1                                                # answer rows incl. [SEP]
    c = 1 + 4 + 3
    Lr = c + A                                                         # first copy row
    checked = 0
    for n in range(1, A):
        for g in range(0, A - n):
            for i in range(2 * (g + 1)):
                j, kind = divmod(i, 2)
                row = (Lr + n + j) if kind else (c + n - 1 + j)        # copy row of step n + j | answer row n - 1 + j
                col_of = lambda r: (Lr + n + r // 2) if r % 2 else (c + n - 1 + r // 2)   # noqa: E731
                keys = set(range(1, c)) | {c + r for r in range(n - 1)} | {col_of(r) for r in pair_keys(i)}
                assert keys == set(np.nonzero(m[row])[0].tolist()), (n, g, i)
                checked += 1
    assert checked > 200


# ---------------------------------------------------------------------------------------------------------------------------
# the budget
# ---------------------------------------------------------------------------------------------------------------------------
def test_f32_restatement_inside_budget():
    """C_VER by C_DEC's rule: the power of two >= 8 x the worst fp32-restatement / T32 ratio over the new cases."""
    worst = SR.measure()
    print(f"\nattn_verify: worst |fp32 restatement - fp64| / T32 = {worst:.4f} (recorded {SR.VER_MEASURED}), C_VER = {SR.C_VER}")
    assert worst <= SR.VER_MEASURED * 1.0001
    assert SR.C_VER == 2.0 ** math.ceil(math.log2(8 * SR.VER_MEASURED))
    case = SR.truncation_case()
    assert SR.attn_verify(*GR.decode_args(case, GR.decode_views(case)))["nk"].tolist() == [256 + 32 + i // 2 + 1 + i % 2
                                                                                          for i in range(32)] * 3


def test_nr2_is_attn_decode_in_the_restatement():
    case = GR.decode_case(9, 2, 3, 2, 2, 6, [9, 64], [0, 1, 6, 8, -1, 3])
    args = GR.decode_args(case, GR.decode_views(case))
    assert torch.equal(SR.attn_verify(*args)["out"], GR.attn_decode(*args)["out"])
    assert torch.equal(SR.attn_verify_f32(*args), GR.attn_decode_f32(*args))


def test_append_restatement():
    cache = torch.zeros((2, 3, 4, 16), dtype=torch.bfloat16)
    buf = torch.arange(2 * 12 * 24, dtype=torch.float32).reshape(2 * 12, 24).to(torch.bfloat16)
    want, po = SR.kv_cache_append(cache, buf[:, 8:], [2, 0, 5], [1, 4, 3], 2, 3, 4, 16, 2, 12 * 24, 4, 2)
    assert po.tolist() == [3, 4, 4]
    assert torch.equal(want[1, 0, 2], buf[12 + 2, 8:]) and torch.equal(want[0, 2, 3], buf[8, 8:])
    assert int((want != 0).any(-1).sum()) == 2 * 3


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
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
    G, T, R = 2, 32, 5
    args = (torch.randint(1000, (G, T)), torch.randn(G, R, 192), torch.rand(G, R, 5), [6, 9])
    return dict(model=model, draft=frozen_reference(model), args=args)


def test_plain_calls_do_not_know_the_module(w):
    import inspect
    from unimm_amd import generation
    from unimm_amd.modeling import BertForMultiModalPreTraining, VisualDialogEncoder
    for fn in (generation.generate_answers, BertForMultiModalPreTraining.generate_answers, VisualDialogEncoder.generate_answers):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ["draft", "draft_len"], names
        p = inspect.signature(fn).parameters
        assert p["draft"].default is None and p["draft_len"].default == 4
    from unimm_amd.generation import GeneratedAnswers
    assert GeneratedAnswers(*[None] * 5).speculation is None


REFUSALS = (
    ("beams", dict(beams=2), "beams = 1"),
    ("samples", dict(samples=2), "speculative sampling"),
    ("ngram", dict(no_repeat_ngram_size=2), "history rules"),
    ("penalty", dict(repetition_penalty=1.2), "history rules"),
    ("scope", dict(repeat_scope="dialog"), "history rules"),
    ("len0", dict(draft_len=0), "draft_len"),
    ("len16", dict(draft_len=16), "draft_len"),
    ("lenf", dict(draft_len=2.0), "draft_len"),
    ("self", dict(draft="self"), "the model itself"),
    ("engine", dict(draft="engine"), "the model itself"),
    ("class", dict(draft=torch.nn.Linear(2, 2)), "BertForMultiModalPreTraining or a VisualDialogEncoder"),
    ("device", dict(draft="meta"), "move it with"),
    ("fp32x3", dict(draft="fp32x3"), "bf16 engine"),
    ("coatt", dict(draft="nocoatt"), "connection layers"),
    ("head", dict(draft="head"), "head size 32"),
    ("vocab", dict(draft=dict(vocab_size=1064)), "vocab_size"),
    ("feat", dict(draft=dict(v_feature_size=128)), "v_feature_size"),
    ("types", dict(draft=dict(type_vocab_size=3)), "type_vocab_size"),
    ("pos", dict(draft=dict(max_position_embeddings=256)), "max_position_embeddings"),
)


@pytest.mark.parametrize("name,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_before_anything_is_staged(w, monkeypatch, name, kw, msg):
    import copy
    from unimm_amd import lib as L
    from unimm_amd.engine import Engine

    def never(*a, **k):
        raise AssertionError("a refused request reached the engine")
    monkeypatch.setattr(L, "_call", never)
    monkeypatch.setattr(L, "lib", never)
    monkeypatch.setattr(Engine, "ensure", never)
    monkeypatch.setattr(Engine, "stage_host_inputs", never)
    kw = dict(kw)
    d = kw.pop("draft", w["draft"])
    if d == "self":
        d = w["model"]
    elif d == "engine":
        d = copy.copy(w["draft"])
        d._engine = w["model"]._engine
    elif d == "meta":
        d = copy.deepcopy(w["draft"]).to("meta")
    elif d == "fp32x3":
        d = _make("fp32x3")
    elif d == "nocoatt":
        d = copy.deepcopy(w["draft"])
        d.config = copy.copy(d.config)
        d.config.with_coattention = False
    elif d == "head":
        d = _make(num_attention_heads=4)
    elif isinstance(d, dict):
        d = _make(**d)
    with pytest.raises(ValueError, match=msg):
        w["model"].generate_answers(*w["args"], draft=d, **kw)


def test_a_shallower_draft_of_other_widths_is_admitted(w):
    """depth, widths, head counts and the connection schedule are the draft's own: the checks pass and the call goes on to
    the engine (which refuses a CPU model)"""
    from unimm_amd import lib as L
    from unimm_amd.speculative import check_draft
    d = _make(num_hidden_layers=2, v_num_hidden_layers=1, t_biattention_id=[1], v_biattention_id=[0], hidden_size=64,
              num_attention_heads=1, intermediate_size=128)
    assert check_draft(w["model"], d, 15, 1, 0, 0, 1.0, "answer") is d
    with pytest.raises(L.UnimmHipError):
        w["model"].generate_answers(*w["args"], draft=d)
