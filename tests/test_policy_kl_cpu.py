"""The host side of the KL leash of policy-gradient fine-tuning (unimm_amd/policy.py: PolicyObjective.kl_coef, lm_reference,
frozen_reference) and the float64 restatement the GPU tests compare the kernels with (tests/policy_kl_ref.py): the restatement
against torch.autograd, the properties of the KL term, and every refusal that needs no device."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import policy_kl_ref as KR
from tests import policy_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def rows(seed, n=24, V=50):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, V)) * 2
    zr = z + rng.standard_normal((n, V)) * 0.7
    y = rng.integers(0, V, n)
    y[[3, 11]] = -1
    A = rng.standard_normal(n)
    A[[1, 7]] = 0.0
    fw0 = PR.forward(z, y, np.zeros(n), None, PR.LOGP, math.inf, 0.0)
    shift = np.array([(-0.5, 0.0, 0.5)[i % 3] for i in range(n)])
    return z, zr, y, A, fw0["logp"] - shift


@pytest.mark.parametrize("mode,eps", [(PR.LOGP, math.inf), (PR.RATIO, 0.2)])
@pytest.mark.parametrize("beta", [0.0, 0.01])
@pytest.mark.parametrize("kl_coef", [0.0, 0.05, 1.0])
def test_restated_gradient_equals_autograd(mode, eps, beta, kl_coef):
    z, zr, y, A, b = rows(int(mode * 7 + beta * 1000 + kl_coef * 100))
    fw = KR.forward(z, zr, y, A, b, mode, eps, beta, kl_coef)
    grad, g_adv, g_ent, g_kl = KR.backward(fw, y, beta, gs=0.5)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    zrt = torch.tensor(zr, dtype=torch.float64, requires_grad=True)
    loss = 0.5 * KR.torch_objective(zt, zrt, y, A, b, mode, eps, beta, kl_coef)
    loss.backward()
    assert abs(float(loss.detach()) - 0.5 * fw["rowloss"].sum()) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    assert np.abs(zt.grad.numpy() - grad).max() <= 1e-13
    assert zrt.grad is None                                          # nothing flows into the reference
    assert (grad[[3, 11]] == 0).all() and (fw["rowloss"][[3, 11]] == 0).all() and (fw["kl"][[3, 11]] == 0).all()
    # the pieces: without the penalty the restatement IS policy_ref's, and the KL term is its own addend
    base = PR.forward(z, y, A, b, mode, eps, beta)
    gb, _, _ = PR.backward(base, y, beta, 0.5)
    assert np.array_equal(fw["rowloss_pg"], base["rowloss"]) and np.array_equal(g_adv + g_ent, gb)
    if kl_coef == 0:
        assert np.array_equal(fw["rowloss"], base["rowloss"]) and np.array_equal(grad, gb) and (g_kl == 0).all()
    else:
        live = fw["has"]
        assert np.abs(g_kl[live]).max() > 1e-4                       # A == 0 rows (1, 7) included: the term is not switched off
        assert np.abs(g_kl[[1, 7]]).max() > 1e-4
        assert np.abs(g_kl.sum(1)).max() <= 1e-14                    # a softmax gradient: sums to zero over the row


def test_kl_properties():
    z, zr, y, A, b = rows(5)
    fw = KR.forward(z, zr, y, A, b, PR.LOGP, math.inf, 0.0, 1.0)
    assert (fw["kl_raw"] > 0).all()                                   # KL >= 0, > 0 for distinct distributions
    # against the textbook form on the two softmaxes
    p, pr = torch.softmax(torch.tensor(z), -1), torch.softmax(torch.tensor(zr), -1)
    assert np.abs((p * (p / pr).log()).sum(-1).numpy() - fw["kl_raw"]).max() <= 1e-13
    # zr = z + const is the same distribution: KL == 0 (to rounding), and so is its gradient
    for const in (0.0, 3.25, -100.0):
        same = KR.forward(z, z + const, y, A, b, PR.LOGP, math.inf, 0.0, 1.0)
        assert np.abs(same["kl_raw"]).max() <= 1e-12
        assert np.abs(KR.backward(same, y, 0.0, 1.0)[3]).max() <= 1e-12
        if const == 0.0:
            assert (same["kl_raw"] == 0).all() and np.array_equal(same["ref_lse"], same["lse"])


def test_minus_infinity_contract():
    """z_i = -inf: p_i = 0, exactly 0 in KL and in its gradient element, whatever zr_i holds (finite or -inf)."""
    rng = np.random.default_rng(0)
    z = rng.standard_normal((4, 12))
    zr = z + rng.standard_normal((4, 12)) * 0.3
    z[0, 3] = z[1, 5] = z[2, 0] = z[2, 7] = -np.inf
    zr[1, 5] = zr[2, 7] = -np.inf                                     # -inf under a -inf; zr[0, 3], zr[2, 0] stay finite
    y = np.array([3, 2, 1, -1])                                       # row 0: -inf ON the label
    for mode in (PR.LOGP, PR.RATIO):
        fw = KR.forward(z, zr, y, np.array([0.0, 1.0, -1.0, 2.0]), np.full(4, -2.0), mode, 0.2, 0.01, 0.5)
        grad, _, _, g_kl = KR.backward(fw, y, 0.01, 0.5)
        assert np.isfinite(grad).all() and np.isfinite(fw["kl_raw"]).all() and np.isfinite(fw["ref_lse"]).all()
        assert (fw["kl_raw"][:3] > 0).all() and fw["kl"][3] == 0
        for r, c in ((0, 3), (1, 5), (2, 0), (2, 7)):
            assert g_kl[r, c] == 0.0 and fw["dk"][r, c] == 0.0
        # ... and the KL is that of the finite columns alone
        keep = np.isfinite(z[1])
        alone = KR.forward(z[1:2, keep], zr[1:2, keep], np.array([1]), np.ones(1), None, PR.LOGP, math.inf, 0.0, 0.5)
        assert abs(alone["kl_raw"][0] - fw["kl_raw"][1]) <= 1e-14


# ---------------------------------------------------------------------------------------------------------------------------
# the objective and the refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_objective_kl_coef():
    from unimm_amd.policy import PolicyObjective
    assert PolicyObjective() == PolicyObjective("logp", math.inf, 0.0)              # existing call forms are unaffected
    assert PolicyObjective() == PolicyObjective("logp", math.inf, 0.0, 0.0) and PolicyObjective().kl_coef == 0.0
    assert PolicyObjective("ratio", 0.2, 0.01, 0.05).kl_coef == 0.05 and PolicyObjective(kl_coef=1).kl_coef == 1
    for bad in (-0.1, math.inf, -math.inf, math.nan):
        with pytest.raises(ValueError, match="kl_coef"):
            PolicyObjective(kl_coef=bad)
    import unimm_amd
    assert unimm_amd.PolicyObjective is PolicyObjective and "frozen_reference" in unimm_amd.__all__


def _make(wrapper, dtype="bf16", **over):
    from unimm_amd import BertConfig, BertForMultiModalPreTraining, VisualDialogEncoder
    cfg_path = os.path.join(ROOT, "tests", "golden", "small_config.json")
    cfg = json.load(open(cfg_path))
    if wrapper and not over:
        return VisualDialogEncoder(cfg_path, compute_dtype=dtype)
    cfg.update(over)
    return BertForMultiModalPreTraining(BertConfig.from_dict(cfg), compute_dtype=dtype)


def test_frozen_reference_is_a_detached_eval_copy():
    from unimm_amd.policy import frozen_reference
    for wrapper in (False, True):
        model = _make(wrapper)
        model.train()
        pre = model.bert_pretrained if wrapper else model
        pre.set_dropout_seed(77, 5)
        ref = frozen_reference(model)
        rpre = ref.bert_pretrained if wrapper else ref
        assert type(ref) is type(model) and ref is not model and not ref.training and model.training
        assert rpre.engine is not pre.engine and rpre.engine.model is rpre and rpre.engine.cfg is rpre.config
        assert (rpre.engine.seed, rpre.engine.step) == (77, 5) and type(rpre.engine) is type(pre.engine)
        mine, theirs = dict(model.named_parameters()), dict(ref.named_parameters())
        assert mine.keys() == theirs.keys() and len(mine) > 20
        for k, p in mine.items():
            q = theirs[k]
            assert not q.requires_grad and p.requires_grad and q.grad is None
            assert torch.equal(p, q) and p.data_ptr() != q.data_ptr()
        # the tied decoder stays tied in the copy
        assert rpre.cls.predictions.decoder.weight is rpre.bert.embeddings.word_embeddings.weight \
            if hasattr(rpre.cls.predictions, "decoder") else True
        with torch.no_grad():
            next(iter(model.parameters())).add_(1.0)
        assert not torch.equal(next(iter(model.parameters())), next(iter(ref.parameters())))


@pytest.mark.parametrize("wrapper", [False, True])
def test_reference_refusals_need_no_device(wrapper):
    """forward / forward_backward of both classes refuse before anything touches a device: CPU tensors, no library call."""
    from unimm_amd.policy import PolicyObjective, frozen_reference
    model = _make(wrapper)
    ref = frozen_reference(model)
    B, T = 2, 16
    ids = torch.zeros((B, T), dtype=torch.int64)
    feat, loc = torch.zeros((B, 3, 8)), torch.zeros((B, 3, 5))
    adv = torch.zeros((B, T))
    lab = torch.full((B, T), -1)
    kl = PolicyObjective(kl_coef=0.05)
    small = json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json")))
    cases = [
        (dict(lm_advantage=adv, lm_objective=kl), "pass lm_reference"),                       # kl_coef > 0 without a reference
        (dict(lm_reference=ref), "pass lm_advantage"),                                          # a reference without an advantage
        (dict(lm_reference=ref, lm_weight=torch.ones((B, T), dtype=torch.int64)), "pass lm_advantage"),
        (dict(lm_advantage=adv, lm_objective=kl, lm_reference=model), "frozen_reference"),      # the trained model itself
        (dict(lm_advantage=adv, lm_reference=model), "frozen_reference"),                        # ... also with kl_coef == 0
        (dict(lm_advantage=adv, lm_objective=kl, lm_reference=_make(False, vocab_size=small["vocab_size"] + 8)), "vocab_size"),
        (dict(lm_advantage=adv, lm_objective=kl, lm_reference=_make(False, intermediate_size=small["intermediate_size"] * 2)),
         "intermediate_size"),
        (dict(lm_advantage=adv, lm_objective=kl, lm_reference=_make(False, fixed_t_layer=1)), "fixed_t_layer"),
        (dict(lm_advantage=adv, lm_objective=kl, lm_reference=_make(wrapper, "fp32x3")), "bf16 engine"),
        (dict(lm_advantage=adv, lm_objective=kl, lm_reference=frozen_reference(model).to("meta")), "is on meta"),
        (dict(lm_advantage=adv, lm_objective=kl, lm_reference="checkpoint.bin"), "must be a BertForMultiModalPreTraining"),
    ]
    if wrapper:
        cases.append((dict(lm_advantage=adv, lm_objective=kl, lm_reference=model.bert_pretrained), "frozen_reference"))
    train = dict(next_sentence_label=torch.zeros(B, dtype=torch.int64), image_target=torch.zeros((B, 3, 4)))
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            model(ids, feat, loc, masked_lm_labels=lab, **train, **kw)
        with pytest.raises(ValueError, match=msg):
            model.forward_backward(ids, feat, loc, (1.0, 0.0, 0.0), masked_lm_labels=lab, **train, **kw)


def test_check_reference_accepts_and_ignores():
    """what passes: a frozen copy of either class for a model of either class; with kl_coef == 0 it is accepted and ignored"""
    from unimm_amd.policy import PolicyObjective, check_policy_inputs, check_reference, frozen_reference
    model, enc = _make(False), _make(True)
    for ref in (frozen_reference(model), frozen_reference(enc)):
        pre = ref.bert_pretrained if hasattr(ref, "bert_pretrained") else ref
        assert check_reference(model, ref, PolicyObjective(kl_coef=0.5)) is pre          # unwrapped to the pre-training model
        assert check_reference(model, ref, PolicyObjective()) is None                     # kl_coef == 0: no second forward
    assert check_reference(model, None, PolicyObjective()) is None and check_reference(model, None, None) is None
    adv = torch.zeros((2, 16))
    obj = check_policy_inputs((2, 16), adv, None, PolicyObjective(kl_coef=0.5), None, "bf16", lm_reference=frozen_reference(model))
    assert obj.kl_coef == 0.5
    assert check_policy_inputs((2, 16), adv, None, None, None, "bf16") == PolicyObjective()      # the existing call form


def test_self_critical_step_takes_a_reference():
    import inspect
    from unimm_amd import trainer
    sig = inspect.signature(trainer.self_critical_step)
    assert sig.parameters["reference"].default is None and sig.parameters["reference"].kind is inspect.Parameter.KEYWORD_ONLY
