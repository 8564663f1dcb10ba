"""The host side of policy-gradient fine-tuning (unimm_amd/policy.py) and the float64 restatement the GPU tests compare the
kernels with (tests/policy_ref.py): the restatement against torch.autograd, the assembly of the sampled answers against
oracle.masks.encode_gen, the advantage arithmetic and every refusal that needs no device."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import policy_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEP, MASK = 102, 103


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,eps", [(PR.LOGP, math.inf), (PR.RATIO, math.inf), (PR.RATIO, 0.2)])
@pytest.mark.parametrize("beta", [0.0, 0.01])
def test_restated_gradient_equals_autograd(mode, eps, beta):
    rng = np.random.default_rng(int(mode * 7 + beta * 1000 + (0 if math.isinf(eps) else 3)))
    n, V = 24, 50
    z = rng.standard_normal((n, V)) * 2
    y = rng.integers(0, V, n)
    y[[3, 11]] = -1
    A = rng.standard_normal(n)
    A[[1, 7]] = 0.0
    fw0 = PR.forward(z, y, np.zeros(n), None, PR.LOGP, math.inf, 0.0)
    # behaviour log-probabilities that put r below 1 - eps, inside and above 1 + eps, for both signs of A
    shift = np.array([(-0.5, 0.0, 0.5)[i % 3] for i in range(n)])
    b = fw0["logp"] - shift                                         # r = e^shift: 0.61, 1, 1.65
    fw = PR.forward(z, y, A, b, mode, eps, beta)
    grad, _, _ = PR.backward(fw, y, beta, gs=1.0)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    loss = PR.torch_objective(zt, y, A, b, mode, eps, beta)
    loss.backward()
    assert abs(float(loss.detach()) - fw["rowloss"].sum()) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    assert np.abs(zt.grad.numpy() - grad).max() <= 1e-13
    assert (grad[[3, 11]] == 0).all() and (fw["rowloss"][[3, 11]] == 0).all()
    if mode == PR.RATIO and not math.isinf(eps):
        act = fw["clipped"]
        assert act.sum() >= 4 and (~act & fw["has"] & (A != 0)).sum() >= 4          # clip active and inactive
        if beta == 0.0:
            assert (grad[act] == 0).all()
    else:
        assert not fw["clipped"].any()


def test_restatement_with_infinite_logits_has_no_nan():
    rng = np.random.default_rng(0)
    z = rng.standard_normal((4, 12))
    z[0, 3] = z[1, 5] = z[2, 0] = z[2, 7] = -np.inf
    y = np.array([3, 2, 1, -1])                                       # row 0: -inf ON the label
    for mode in (PR.LOGP, PR.RATIO):
        fw = PR.forward(z, y, np.array([0.0, 1.0, -1.0, 2.0]), np.full(4, -2.0), mode, 0.2, 0.01)
        grad, _, _ = PR.backward(fw, y, 0.01, 0.5)
        assert np.isfinite(grad).all() and np.isfinite(fw["ent"]).all() and np.isfinite(fw["rowloss"]).all()
        assert grad[0, 3] == 0.0 and fw["rownll"][0] == np.inf


# ---------------------------------------------------------------------------------------------------------------------------
# the sampled answers as a training batch
# ---------------------------------------------------------------------------------------------------------------------------
def dialogs(G, T, seed):
    """G contexts laid out by encode_gen (as tests/test_gpu_generate.py::make_dialogs) -> ids, segments, positions, c, utterances"""
    from oracle import masks as OM
    rng = np.random.default_rng(seed)
    ids, tt, pp = (np.zeros((G, T), np.int64) for _ in range(3))
    c = np.zeros(G, np.int64)
    utts = []
    for g in range(G):
        u = [rng.integers(110, 1000, int(rng.integers(1, 6))).tolist() for _ in range(int(rng.integers(1, 5)))]
        start = int(rng.integers(0, 2))
        enc = OM.encode_gen(u + [[]], start_segment=start, max_seq_len=T)
        cg = 1 + sum(len(x) + 1 for x in u)
        ids[g, :cg], tt[g, :cg], pp[g, :cg] = enc["tokens"][0, :cg], enc["segments"][0, :cg], enc["positions"][0, :cg]
        c[g] = cg
        utts.append((u, start))
    return ids, tt, pp, c, utts


def answers_for(c, T, N, W, seed):
    """N answers per dialog (tokens + [SEP], zero-padded to W): random lengths, one at the dialog's limit, one of length 0."""
    from unimm_amd.generation import GeneratedAnswers, answer_limits
    rng = np.random.default_rng(seed)
    G = len(c)
    lim = answer_limits(c, T, W - 1)
    tok = np.zeros((G, N, W), np.int64)
    ln = np.zeros((G, N), np.int64)
    for g in range(G):
        for j in range(N):
            if j == 0:
                k = int(lim[g]) + 1                                   # the dialog's limit of tokens + [SEP]
            elif j == 1 and g % 2 == 0:
                k = 0                                                 # beam padding
            else:
                k = int(rng.integers(1, lim[g] + 2))
            if k:
                tok[g, j, :k - 1] = rng.integers(110, 1000, k - 1)
                tok[g, j, k - 1] = SEP
            ln[g, j] = k
    z = torch.zeros((G, N, W))
    return GeneratedAnswers(tokens=torch.from_numpy(tok), lengths=torch.from_numpy(ln), scores=torch.zeros(G, N),
                            logp=torch.zeros(G, N), step_logp=z, step_logq=z.clone())


def test_sampled_training_batch_equals_encode_gen():
    from oracle import masks as OM
    from unimm_amd import policy as P
    G, T, N, W = 5, 48, 4, 9
    ids, tt, pp, c, utts = dialogs(G, T, seed=4)
    ans = answers_for(c, T, N, W, seed=5)
    sb = P.sampled_training_batch(torch.from_numpy(ids), torch.from_numpy(tt), torch.from_numpy(pp), c, ans, T)
    keep = [(g, j) for g in range(G) for j in range(N) if int(ans.lengths[g, j]) > 0]
    assert 0 < len(keep) < G * N and sb.kept.tolist() == [g * N + j for g, j in keep]           # the length-0 drop
    assert sb.image_index.tolist() == [g for g, _ in keep] and sb.shape == (G, N)
    at_limit = 0
    txt, co = sb.attention_mask.dense(T)
    for k, (g, j) in enumerate(keep):
        n = int(ans.lengths[g, j])
        u, start = utts[g]
        enc = OM.encode_gen(u + [ans.tokens[g, j, :n - 1].tolist()], start_segment=start, max_seq_len=T)
        assert (sb.input_ids[k].numpy() == enc["tokens"][0]).all()
        assert (sb.token_type_ids[k].numpy() == enc["segments"][0]).all()
        assert (sb.position_ids[k].numpy() == enc["positions"][0]).all()
        assert (sb.masked_lm_labels[k].numpy() == enc["labels"][0]).all()
        assert (txt[k].numpy() == enc["txt_attention_mask"][0].astype(bool)).all()
        assert (co[k].numpy() == enc["co_attention_mask"][0].astype(bool)).all()
        assert (sb.copy_rows[k].numpy() == (enc["labels"][0] != -1)).all() and int(sb.copy_rows[k].sum()) == n
        at_limit += n - 1 == min(W - 1, (T - int(c[g])) // 2 - 1)
    assert at_limit >= G                                             # an answer that reaches its dialog's limit is included
    assert (sb.attention_mask.mode == 1).all()
    with pytest.raises(ValueError, match="more than T"):
        P.sampled_training_batch(torch.from_numpy(ids), torch.from_numpy(tt), torch.from_numpy(pp), c, ans, int(c.max()) + 3)


def test_spread_and_advantage():
    from unimm_amd import policy as P
    G, T, N, W = 3, 40, 3, 6
    ids, tt, pp, c, _ = dialogs(G, T, seed=1)
    ans = answers_for(c, T, N, W, seed=2)
    sb = P.sampled_training_batch(ids, tt, pp, c, ans, T)
    per_seq = torch.arange(G * N, dtype=torch.float32).view(G, N) + 1
    out = P.spread(per_seq, sb)
    assert out.dtype == torch.float32 and out.shape == sb.copy_rows.shape
    per_tok = torch.arange(G * N * W, dtype=torch.float32).view(G, N, W) + 0.5
    out_t = P.spread(per_tok, sb)
    for k, f in enumerate(sb.kept.tolist()):
        g, j = divmod(f, N)
        rows = sb.copy_rows[k]
        n = int(rows.sum())
        assert (out[k][rows] == per_seq[g, j]).all() and (out[k][~rows] == 0).all()
        assert torch.equal(out_t[k][rows], per_tok[g, j, :n]) and (out_t[k][~rows] == 0).all()
    with pytest.raises(ValueError):
        P.spread(torch.zeros(G + 1, N), sb)
    r = torch.tensor([[1.0, 2.0, 6.0], [0.0, 0.0, 3.0]])
    assert torch.equal(P.self_critical_advantage(r, None), r)
    assert torch.equal(P.self_critical_advantage(r, torch.tensor([2.0, -1.0])), torch.tensor([[-1.0, 0.0, 4.0], [1.0, 1.0, 4.0]]))
    # leave-one-out: sample j against the mean of the OTHER samples of its dialog
    assert torch.equal(P.self_critical_advantage(r, "mean"), torch.tensor([[1 - 4.0, 2 - 3.5, 6 - 1.5], [-1.5, -1.5, 3.0]]))
    assert abs(float(P.self_critical_advantage(r, "mean").sum(1).abs().max())) <= 1e-6      # sums to zero per dialog
    with pytest.raises(ValueError, match="N >= 2"):
        P.self_critical_advantage(r[:, :1], "mean")
    with pytest.raises(ValueError):
        P.self_critical_advantage(r, "median")
    with pytest.raises(ValueError):
        P.self_critical_advantage(r, torch.zeros(3))


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_objective_refusals():
    from unimm_amd.policy import PolicyObjective
    assert PolicyObjective() == PolicyObjective("logp", math.inf, 0.0)
    for kw in (dict(mode="ppo"), dict(clip_eps=-0.1), dict(clip_eps=float("nan")), dict(entropy_coef=math.inf)):
        with pytest.raises(ValueError):
            PolicyObjective(**kw)


@pytest.mark.parametrize("wrapper", [False, True])
def test_model_refusals_need_no_device(wrapper, tmp_path):
    """forward / forward_backward of both classes refuse before anything touches a device: CPU tensors, no library call."""
    from unimm_amd import BertConfig, BertForMultiModalPreTraining, VisualDialogEncoder
    from unimm_amd.policy import PolicyObjective
    cfg_path = os.path.join(ROOT, "tests", "golden", "small_config.json")

    def make(dtype="bf16"):
        if wrapper:
            return VisualDialogEncoder(cfg_path, compute_dtype=dtype)
        return BertForMultiModalPreTraining(BertConfig.from_dict(json.load(open(cfg_path))), compute_dtype=dtype)

    model = make()
    B, T = 2, 16
    ids = torch.zeros((B, T), dtype=torch.int64)
    feat, loc = torch.zeros((B, 3, 8)), torch.zeros((B, 3, 5))
    adv = torch.zeros((B, T))
    lab = torch.full((B, T), -1)
    cases = [
        (dict(lm_advantage=adv, lm_weight=torch.ones((B, T), dtype=torch.int64)), "pass one of them"),
        (dict(lm_advantage=adv, lm_objective=PolicyObjective(mode="ratio")), "lm_behaviour_logp"),
        (dict(lm_advantage=adv.reshape(-1)), r"\[B, T\]"),
        (dict(lm_advantage=adv[:, :-1]), r"\[B, T\]"),
        (dict(lm_advantage=adv, lm_behaviour_logp=adv[:1], lm_objective=PolicyObjective(mode="ratio")), r"\[B, T\]"),
        (dict(lm_advantage=adv, lm_objective="logp"), "PolicyObjective"),
        (dict(lm_behaviour_logp=adv), "pass lm_advantage"),
        (dict(lm_objective=PolicyObjective()), "pass lm_advantage"),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            model(ids, feat, loc, masked_lm_labels=lab, **kw)
        with pytest.raises(ValueError, match=msg):
            model.forward_backward(ids, feat, loc, (1.0, 0.0, 0.0), masked_lm_labels=lab, **kw)
    with pytest.raises(ValueError, match="computes no loss"):         # forward without the training inputs would ignore it
        model(ids, feat, loc, masked_lm_labels=lab, lm_advantage=adv)
    x3 = make("fp32x3")
    with pytest.raises(ValueError, match="bf16 engine only"):
        x3(ids, feat, loc, masked_lm_labels=lab, lm_advantage=adv)
    with pytest.raises(ValueError, match="bf16 engine only"):
        x3.forward_backward(ids, feat, loc, (1.0, 0.0, 0.0), masked_lm_labels=lab, lm_advantage=adv)


def test_graph_executor_is_not_eligible_with_an_advantage():
    """graphs.StepGraphs.eligible answers False as soon as the step has a bound objective (the eager step runs)."""
    from unimm_amd import BertConfig, BertForMultiModalPreTraining, graphs
    from unimm_amd.lm_objective import KEY
    from unimm_amd.policy import bind_objective

    class Eng:
        text_priority = False

        class cfg:
            predict_feature = False

    sg = graphs.StepGraphs.__new__(graphs.StepGraphs)
    sg.eng = Eng()
    model = BertForMultiModalPreTraining(BertConfig.from_dict(json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json")))))
    assert sg.eligible({KEY: bind_objective(model, (1, 1), lm_advantage=torch.zeros(1, 1))}, dict(want_seq=False)) is False
