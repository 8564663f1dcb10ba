"""The host side of preference training (unimm_amd/policy.py: PreferenceObjective, PreferenceTargets, candidate_training_batch,
relevance_targets, pair_targets) and the fp64 restatement the GPU tests compare unimm_seq_pref with (tests/pref_ref.py): the
restatement against torch.autograd and the closed forms, and every refusal that needs no device."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import pref_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def case(seed, groups=3, members=5):
    rng = np.random.default_rng(seed)
    B = groups * members + 2
    seq_group = np.concatenate((np.arange(groups * members) % groups, [0, 1]))       # the last two sequences get no row
    nrows = np.concatenate((rng.integers(1, 7, groups * members), [0, 0]))
    row_seq = np.repeat(np.arange(B), nrows)
    row_seq = row_seq[rng.permutation(row_seq.shape[0])]
    n = row_seq.shape[0]
    rownll = rng.gamma(2.0, 1.5, n).astype(np.float32)
    ref = rng.gamma(2.0, 1.5, n).astype(np.float32)
    w = rng.uniform(0, 1, B).astype(np.float32)
    return dict(rownll=rownll, ref=ref, row_seq=row_seq, seq_group=seq_group, w=w, B=B, groups=groups, n=n, nrows=nrows)


@pytest.mark.parametrize("lnorm", [False, True])
@pytest.mark.parametrize("use_ref", [False, True])
def test_restated_loss_and_coefficients_equal_autograd(lnorm, use_ref):
    c = case(3)
    beta = 0.37
    res = PR.seq_pref(c["rownll"], c["ref"] if use_ref else None, c["row_seq"], c["n"], c["seq_group"], c["w"], c["groups"], beta, lnorm)
    logp = torch.tensor(-c["rownll"].astype(np.float64), requires_grad=True)          # log p_y per row
    seq = torch.tensor(c["row_seq"])
    S = torch.zeros(c["B"], dtype=torch.float64).index_add(0, seq, logp)
    R = torch.zeros(c["B"], dtype=torch.float64).index_add(0, seq, torch.tensor(-c["ref"].astype(np.float64))) if use_ref else 0.0
    Ln = torch.tensor(np.maximum(c["nrows"], 1).astype(np.float64))
    z = float(np.float32(beta)) * (S - R) / (Ln if lnorm else 1.0)
    total = 0.0
    for g in range(c["groups"]):
        mem = torch.tensor([j for j in range(c["B"]) if c["seq_group"][j] == g and c["nrows"][j] > 0])
        w = torch.tensor(c["w"].astype(np.float64))[mem]
        loss_g = -(w * torch.log_softmax(z[mem], 0)).sum()
        assert abs(float(loss_g.detach()) - res["group_loss"][g]) <= 1e-12 * max(1.0, abs(float(loss_g.detach())))
        total = total + loss_g
    total.backward()
    # d loss / d log p_y of a row = -c_j of its sequence
    assert np.abs(-logp.grad.numpy() - res["adv"]).max() <= 1e-13
    assert res["alive"].all() and res["alive_inv"] == 1.0 / c["groups"]
    assert np.isnan(res["seq_score"][-2:]).all() and (res["seq_prob"][-2:] == 0).all()
    # sum_j c_j L_j^lam = 0 per group (the softmax's gradient sums to zero)
    for g in range(c["groups"]):
        mem = [j for j in range(c["B"]) if c["seq_group"][j] == g and c["nrows"][j] > 0]
        s = sum(res["c"][j] * (c["nrows"][j] if lnorm else 1.0) for j in mem)
        assert abs(s) <= 1e-14
        assert abs(res["seq_prob"][mem].sum() - 1.0) <= 1e-14


def test_a_pair_with_a_one_hot_target_is_dpo():
    rng = np.random.default_rng(1)
    for lnorm in (False, True):
        rownll, ref = rng.gamma(2.0, 1.5, 9), rng.gamma(2.0, 1.5, 9)
        row_seq = np.array([0, 0, 0, 0, 1, 1, 1, 1, 1])
        res = PR.seq_pref(rownll, ref, row_seq, 9, [0, 0], [1.0, 0.0], 1, 0.25, lnorm)
        Lw, Ll = (4.0, 5.0) if lnorm else (1.0, 1.0)
        zw = 0.25 * (-(rownll[:4].sum()) + ref[:4].sum()) / Lw
        zl = 0.25 * (-(rownll[4:].sum()) + ref[4:].sum()) / Ll
        want = -float(torch.nn.functional.logsigmoid(torch.tensor(zw - zl, dtype=torch.float64)))
        assert abs(res["group_loss"][0] - want) <= 1e-14 and abs(PR.mean_loss(res) - want) <= 1e-14
        sig = 1.0 / (1.0 + math.exp(zw - zl))                                         # sigmoid(z_l - z_w) = 1 - P_w
        assert abs(res["c"][0] - 0.25 * sig / Lw) <= 1e-15 and abs(res["c"][1] + 0.25 * sig / Ll) <= 1e-15


def test_rules_of_the_restatement():
    c = case(5)
    one = PR.seq_pref([1.5, 2.5], None, [0, 0], 2, [0], [0.7], 1, 0.1, False)          # a one-member group: loss 0, c = 0
    assert one["group_loss"][0] == 0 and (one["adv"] == 0).all() and one["seq_prob"][0] == 1.0 and one["alive"][0]
    w = c["w"].copy()
    w[c["seq_group"] == 1] = 0                                                          # all-zero weights: dead, loss 0, adv 0
    w[np.flatnonzero(c["seq_group"] == 2)[0]] = np.nan                                  # a NaN weight: dead, NaN loss
    res = PR.seq_pref(c["rownll"], None, c["row_seq"], c["n"], c["seq_group"], w, 3, 0.1, False)
    assert list(res["alive"]) == [True, False, False] and res["alive_inv"] == 1.0
    assert res["group_loss"][1] == 0 and np.isnan(res["group_loss"][2]) and res["group_loss"][0] > 0
    assert (res["adv"][np.isin(c["seq_group"][c["row_seq"]], (1, 2))] == 0).all()
    neg = w.copy()
    neg[np.flatnonzero(c["seq_group"] == 0)[1]] = -1.0
    assert np.isnan(PR.seq_pref(c["rownll"], None, c["row_seq"], c["n"], c["seq_group"], neg, 3, 0.1, False)["alive_inv"])
    # rows past the device count, sequences and groups out of range
    part = PR.seq_pref(c["rownll"], None, c["row_seq"], 5, c["seq_group"], c["w"], 3, 0.1, False)
    assert (part["adv"][5:] == 0).all() and part["written_rows"] == 5
    empty = PR.seq_pref(c["rownll"], None, c["row_seq"], 0, c["seq_group"], c["w"], 3, 0.1, False)
    assert np.isnan(empty["alive_inv"]) and (empty["group_loss"] == 0).all()
    rs = c["row_seq"].copy()
    rs[:3] = (-1, c["B"], 10 ** 9)
    sg = c["seq_group"].copy()
    sg[4] = 7
    res = PR.seq_pref(c["rownll"], None, rs, c["n"], sg, c["w"], 3, 0.1, False)
    assert (res["adv"][:3] == 0).all() and res["seq_prob"][4] == 0 and (res["adv"][rs == 4] == 0).all()
    big = PR.seq_pref(np.ones(129), None, np.arange(129), 129, np.zeros(129, int), np.ones(129), 1, 0.1, False)
    assert np.isnan(big["group_loss"][0]) and (big["adv"] == 0).all() and np.isnan(big["alive_inv"])
    sat = PR.seq_pref([1.0, 3.0], None, [0, 1], 2, [0, 0], [1.0, 0.0], 1, 1e4, False)  # z difference 2e4
    assert list(sat["seq_prob"]) == [1.0, 0.0] and sat["group_loss"][0] == 0 and (sat["adv"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the batch and the targets
# ---------------------------------------------------------------------------------------------------------------------------
def test_candidate_batch_equals_the_sampled_batch_of_the_same_tokens():
    from unimm_amd.generation import GeneratedAnswers
    from unimm_amd.policy import SEP, candidate_training_batch, sampled_training_batch
    rng = np.random.default_rng(2)
    G, N, W, T = 3, 4, 7, 40
    ctx = np.array([9, 12, 5])
    ids = torch.from_numpy(rng.integers(1000, 2000, (G, T)))
    tt = torch.from_numpy(rng.integers(0, 2, (G, T)))
    pp = torch.arange(T).repeat(G, 1)
    lengths = torch.tensor([[3, 1, 0, 7], [2, 2, 5, 4], [0, 6, 1, 3]])
    tokens = torch.zeros((G, N, W), dtype=torch.int64)
    for g in range(G):
        for j in range(N):
            n = int(lengths[g, j])
            if n:
                tokens[g, j, :n - 1] = torch.from_numpy(rng.integers(2000, 3000, n - 1))
                tokens[g, j, n - 1] = SEP
    zeros = torch.zeros((G, N))
    ga = GeneratedAnswers(tokens=tokens, lengths=lengths, scores=zeros, logp=zeros, step_logp=torch.zeros((G, N, W)))
    a = candidate_training_batch(ids, tt, pp, ctx, tokens, lengths, T)
    b = sampled_training_batch(ids, tt, pp, ctx, ga, T)
    for k in ("input_ids", "token_type_ids", "position_ids", "masked_lm_labels", "image_index", "copy_rows", "kept"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for k in ("mode", "length", "answer"):
        assert np.array_equal(getattr(a.attention_mask, k), getattr(b.attention_mask, k)), k
    assert a.shape == b.shape == (G, N) and a.input_ids.shape[0] == 10 and a.kept.tolist() == [0, 1, 3, 4, 5, 6, 7, 9, 10, 11]
    assert a.copy_rows.sum(1).tolist() == [3, 1, 7, 2, 2, 5, 4, 6, 1, 3]
    with pytest.raises(ValueError, match="answer_lengths"):
        candidate_training_batch(ids, tt, pp, ctx, tokens, lengths[:, :3], T)
    with pytest.raises(ValueError, match="answer_lengths"):
        candidate_training_batch(ids, tt, pp, ctx, tokens, lengths + 5, T)


def test_targets():
    from unimm_amd.policy import PreferenceTargets, pair_targets, relevance_targets
    rel = torch.tensor([[0.0, 1.0, 0.5], [0.2, 0.2, 0.2]])
    t = relevance_targets(rel)
    assert t.dtype == torch.float32 and torch.allclose(t, torch.softmax(rel, 1)) and torch.allclose(t.sum(1), torch.ones(2))
    assert torch.allclose(relevance_targets(rel, temperature=0.5), torch.softmax(rel / 0.5, 1))
    assert torch.allclose(t[1], torch.full((3,), 1 / 3))
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="temperature"):
            relevance_targets(rel, temperature=bad)
    with pytest.raises(ValueError, match=r"\[G, N\]"):
        relevance_targets(rel[0])
    p = pair_targets([2, 0], 3)
    assert p.dtype == torch.float32 and p.tolist() == [[0, 0, 1], [1, 0, 0]]
    for bad in ([3], [-1]):
        with pytest.raises(ValueError, match="chosen"):
            pair_targets(bad, 3)
    tg = PreferenceTargets(torch.tensor([0, 0, 2]), torch.tensor([1.0, 0.0, 0.5]))
    assert len(tg) == 3 and tg.groups == 3 and tg.group.dtype == np.int64 and tg.weight.dtype == np.float32
    with pytest.raises(ValueError, match="1-D"):
        PreferenceTargets([[0, 1]], [[1.0, 0.0]])
    with pytest.raises(ValueError, match="integer"):
        PreferenceTargets([0.5, 1.0], [1.0, 0.0])


def test_objective_and_exports():
    import unimm_amd
    from unimm_amd import lib, trainer
    from unimm_amd.policy import PREF_MAX_MEMBERS, PreferenceObjective
    assert PreferenceObjective() == PreferenceObjective(0.1, False) and PreferenceObjective(0.5, True).length_normalize
    for bad in (0.0, -0.1, math.inf, math.nan):
        with pytest.raises(ValueError, match="beta"):
            PreferenceObjective(beta=bad)
    assert unimm_amd.PreferenceObjective is PreferenceObjective and "PreferenceTargets" in unimm_amd.__all__
    assert PREF_MAX_MEMBERS == lib.PREF_MAX_MEMBERS == lib.NDCG_MAX_OPTIONS == PR.MAX_MEMBERS == 128
    assert "unimm_seq_pref" in lib.SIGNATURES and lib.STRUCTS["unimm_seq_pref_args"] is lib.SeqPrefArgs
    import inspect
    sig = inspect.signature(trainer.preference_step)
    assert sig.parameters["objective"].default == PreferenceObjective() and sig.parameters["reference"].default is None
    assert sig.parameters["shared_context"].default is True


def test_header_constants_equal_the_binding():
    from tests import header_reader as HR
    from unimm_amd import lib
    c = HR.constants(open(os.path.join(ROOT, "include", "unimm_hip.h")).read())
    assert (c["UNIMM_PREF_MAX_MEMBERS"], c["UNIMM_PREF_WS_ITEM_BYTES"]) == (lib.PREF_MAX_MEMBERS, lib.PREF_WS_ITEM_BYTES)


# ---------------------------------------------------------------------------------------------------------------------------
# the refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _make(wrapper, dtype="bf16", **over):
    from unimm_amd import BertConfig, BertForMultiModalPreTraining, VisualDialogEncoder
    cfg_path = os.path.join(ROOT, "tests", "golden", "small_config.json")
    cfg = json.load(open(cfg_path))
    if wrapper and not over:
        return VisualDialogEncoder(cfg_path, compute_dtype=dtype)
    cfg.update(over)
    return BertForMultiModalPreTraining(BertConfig.from_dict(cfg), compute_dtype=dtype)


@pytest.mark.parametrize("wrapper", [False, True])
def test_preference_refusals_need_no_device(wrapper):
    """forward / forward_backward of both classes refuse before anything touches a device: CPU tensors, no library call."""
    from unimm_amd.policy import PolicyObjective, PreferenceObjective, PreferenceTargets, frozen_reference
    model = _make(wrapper)
    ref = frozen_reference(model)
    B, T = 4, 16
    ids = torch.zeros((B, T), dtype=torch.int64)
    feat, loc = torch.zeros((B, 3, 8)), torch.zeros((B, 3, 5))
    lab = torch.full((B, T), -1)
    tg = PreferenceTargets([0, 0, 1, 1], [1.0, 0.0, 1.0, 0.0])
    obj = PreferenceObjective()
    small = json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json")))
    broken = PreferenceObjective()
    object.__setattr__(broken, "beta", -1.0)                                                 # past the constructor's own check
    cases = [
        (dict(lm_preference=tg, lm_objective=obj, lm_advantage=torch.zeros((B, T))), "lm_advantage"),
        (dict(lm_preference=tg, lm_objective=obj, lm_weight=torch.ones((B, T), dtype=torch.int64)), "lm_weight"),
        (dict(lm_preference=tg, lm_objective=obj, lm_behaviour_logp=torch.zeros((B, T))), "lm_behaviour_logp"),
        (dict(lm_preference=tg), "PreferenceObjective"),
        (dict(lm_preference=tg, lm_objective=PolicyObjective()), "PreferenceObjective"),
        (dict(lm_objective=obj), "pass lm_advantage"),                                       # the objective without targets
        (dict(lm_preference=([0, 0, 1, 1], [1.0, 0.0, 1.0, 0.0]), lm_objective=obj), "PreferenceTargets"),
        (dict(lm_preference=PreferenceTargets([0, 0, 1], [1.0, 0.0, 1.0]), lm_objective=obj), "one of each per sequence"),
        (dict(lm_preference=PreferenceTargets([0, 0, 1, 1, 1], [1.0, 0.0, 1.0, 0.0, 0.0]), lm_objective=obj), "one of each per"),
        (dict(lm_preference=PreferenceTargets([0, 0, 1, 1], [1.0, -0.5, 1.0, 0.0]), lm_objective=obj), "finite and >= 0"),
        (dict(lm_preference=PreferenceTargets([0, 0, 1, 1], [1.0, math.nan, 1.0, 0.0]), lm_objective=obj), "finite and >= 0"),
        (dict(lm_preference=PreferenceTargets([0, 0, 1, 1], [1.0, math.inf, 1.0, 0.0]), lm_objective=obj), "finite and >= 0"),
        (dict(lm_preference=PreferenceTargets([0, 0, -1, 1], [1.0, 0.0, 1.0, 0.0]), lm_objective=obj), "group id"),
        (dict(lm_preference=tg, lm_objective=broken), "beta"),
        # every refusal of a reference
        (dict(lm_preference=tg, lm_objective=obj, lm_reference=model), "frozen_reference"),
        (dict(lm_preference=tg, lm_objective=obj, lm_reference=_make(False, vocab_size=small["vocab_size"] + 8)), "vocab_size"),
        (dict(lm_preference=tg, lm_objective=obj, lm_reference=_make(False, intermediate_size=small["intermediate_size"] * 2)),
         "intermediate_size"),
        (dict(lm_preference=tg, lm_objective=obj, lm_reference=_make(False, fixed_t_layer=1)), "fixed_t_layer"),
        (dict(lm_preference=tg, lm_objective=obj, lm_reference=_make(wrapper, "fp32x3")), "bf16 engine"),
        (dict(lm_preference=tg, lm_objective=obj, lm_reference=frozen_reference(model).to("meta")), "is on meta"),
        (dict(lm_preference=tg, lm_objective=obj, lm_reference="checkpoint.bin"), "must be a BertForMultiModalPreTraining"),
    ]
    if wrapper:
        cases.append((dict(lm_preference=tg, lm_objective=obj, lm_reference=model.bert_pretrained), "frozen_reference"))
    train = dict(next_sentence_label=torch.zeros(B, dtype=torch.int64), image_target=torch.zeros((B, 3, 4)))
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            model(ids, feat, loc, masked_lm_labels=lab, **train, **kw)
        with pytest.raises(ValueError, match=msg):
            model.forward_backward(ids, feat, loc, (1.0, 0.0, 0.0), masked_lm_labels=lab, **train, **kw)
    with pytest.raises(ValueError, match="train branch"):                                  # a forward that computes no loss
        model(ids, feat, loc, lm_preference=tg, lm_objective=obj)
    with pytest.raises(ValueError, match="pass lm_preference"):                            # the shared schedule without targets
        model(ids, feat, loc, masked_lm_labels=lab, shared_context=[0, 0, 1, 1], **train)
    with pytest.raises(ValueError, match="DialogMaskSpec"):                                # ... and its own conditions with them
        model(ids, feat, loc, masked_lm_labels=lab, shared_context=[0, 0, 1, 1], lm_preference=tg, lm_objective=obj)
    # more than 128 sequences in a group
    Bb = 130
    many = PreferenceTargets([0] * 129 + [1], [1.0] * Bb)
    big = dict(next_sentence_label=torch.zeros(Bb, dtype=torch.int64), image_target=torch.zeros((Bb, 3, 4)))
    with pytest.raises(ValueError, match="at most 128"):
        model.forward_backward(torch.zeros((Bb, T), dtype=torch.int64), torch.zeros((Bb, 3, 8)), torch.zeros((Bb, 3, 5)),
                               (1.0, 0.0, 0.0), masked_lm_labels=torch.full((Bb, T), -1), lm_preference=many, lm_objective=obj, **big)
    # the fp32x3 engine
    x3 = _make(wrapper, "fp32x3")
    with pytest.raises(ValueError, match="bf16 engine only"):
        x3(ids, feat, loc, masked_lm_labels=lab, lm_preference=tg, lm_objective=obj, **train)
    with pytest.raises(ValueError, match="bf16 engine only"):
        x3.forward_backward(ids, feat, loc, (1.0, 0.0, 0.0), masked_lm_labels=lab, lm_preference=tg, lm_objective=obj, **train)


def test_check_reference_takes_a_preference_objective():
    from unimm_amd.policy import PreferenceObjective, check_reference, frozen_reference
    model, enc = _make(False), _make(True)
    for ref in (frozen_reference(model), frozen_reference(enc)):
        pre = ref.bert_pretrained if hasattr(ref, "bert_pretrained") else ref
        assert check_reference(model, ref, PreferenceObjective()) is pre
    assert check_reference(model, None, PreferenceObjective()) is None                     # a reference is optional: R = 0


def test_the_graph_executor_declines_the_step():
    from unimm_amd.graphs import StepGraphs
    from unimm_amd.lm_objective import KEY
    from unimm_amd.policy import PreferenceObjective, PreferenceTargets, bind_objective

    class _Eng:
        text_priority = False

        class cfg:
            predict_feature = False
    sg = StepGraphs.__new__(StepGraphs)
    sg.eng = _Eng()
    bound = bind_objective(_make(False), (1, 16), lm_preference=PreferenceTargets([0], [1.0]), lm_objective=PreferenceObjective())
    assert sg.eligible({KEY: bound}, dict(want_seq=False)) is False
