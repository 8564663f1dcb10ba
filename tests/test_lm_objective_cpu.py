"""`policy.bind_objective`, the one place where the objective arguments of `forward` / `forward_backward` are judged and become
the step's bound objective (unimm_amd/lm_objective.py): what each combination binds, every refusal the policy, KL and
preference CPU suites test by message raised through it with the same message, and the graph executor's one rule.  Host only:
nothing here loads the library or touches a device."""
import json
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = B, T = 2, 16


def _make(dtype="bf16", **over):
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json")))
    cfg.update(over)
    return BertForMultiModalPreTraining(BertConfig.from_dict(cfg), compute_dtype=dtype)


@pytest.fixture(scope="module")
def w():
    """one model, a frozen copy of it, an advantage, preference targets and the two kinds of objective"""
    from unimm_amd.policy import PolicyObjective, PreferenceObjective, PreferenceTargets, frozen_reference
    model = _make()
    return dict(model=model, ref=frozen_reference(model), adv=torch.zeros(SHAPE), tg=PreferenceTargets([0, 0], [1.0, 0.0]),
                kl=PolicyObjective(kl_coef=0.5), pref=PreferenceObjective(), small=model.config)


def bind(w, train_branch=True, model=None, shape=SHAPE, **kw):
    from unimm_amd.policy import bind_objective
    return bind_objective(w["model"] if model is None else model, shape, train_branch, **kw)


def test_the_likelihood_step_binds_nothing(w):
    assert bind(w) is None
    assert bind(w, lm_weight=torch.ones(SHAPE, dtype=torch.int64)) is None
    assert bind(w, train_branch=False) is None                      # an inference forward


def test_an_advantage_binds_the_policy_gradient(w):
    from unimm_amd import lib as L
    from unimm_amd.lm_objective import PolicyGradient
    from unimm_amd.policy import PolicyObjective
    o = bind(w, lm_advantage=w["adv"])
    assert type(o) is PolicyGradient and o.objective == PolicyObjective() and o.reference is None and o.ref is None
    assert o.adv is w["adv"] and o.blogp is None and (o.mode, o.eps, o.beta, o.kl_coef) == (L.PG_LOGP, math.inf, 0.0, 0.0)
    logq = torch.zeros(SHAPE)
    o = bind(w, lm_advantage=w["adv"], lm_behaviour_logp=logq, lm_objective=PolicyObjective("ratio", 0.2, 0.01))
    assert o.blogp is logq and (o.mode, o.eps, o.beta) == (L.PG_RATIO, 0.2, 0.01)
    assert bind(w, lm_advantage=w["adv"], lm_behaviour_logp=logq).blogp is None      # mode "logp" does not read it


def test_the_kl_leash_needs_the_reference_forward_only_with_a_coefficient(w):
    from unimm_amd.lm_objective import PolicyGradient
    from unimm_amd.policy import PolicyObjective
    o = bind(w, lm_advantage=w["adv"], lm_objective=w["kl"], lm_reference=w["ref"])
    assert type(o) is PolicyGradient and o.reference is w["ref"] and o.kl_coef == 0.5 and o.ref is None
    o = bind(w, lm_advantage=w["adv"], lm_objective=PolicyObjective(kl_coef=0.0), lm_reference=w["ref"])
    assert type(o) is PolicyGradient and o.reference is None        # accepted and ignored: no reference forward


def test_targets_bind_the_preference_with_or_without_a_reference(w):
    from unimm_amd.lm_objective import Preference
    from unimm_amd.policy import PreferenceObjective
    o = bind(w, lm_preference=w["tg"], lm_objective=PreferenceObjective(0.5, True))
    assert type(o) is Preference and o.reference is None and o.ref is None
    assert (o.T, o.groups, o.beta, o.lnorm) == (T, 1, 0.5, True) and o.group is w["tg"].group and o.weight is w["tg"].weight
    o = bind(w, lm_preference=w["tg"], lm_objective=w["pref"], lm_reference=w["ref"])
    assert type(o) is Preference and o.reference is w["ref"]


def _broken_beta():
    from unimm_amd.policy import PreferenceObjective
    broken = PreferenceObjective()
    object.__setattr__(broken, "beta", -1.0)                        # past the constructor's own check
    return broken


def _targets(group, weight):
    from unimm_amd.policy import PreferenceTargets
    return PreferenceTargets(group, weight)


def _frozen(model):
    from unimm_amd.policy import frozen_reference
    return frozen_reference(model)


def _ratio():
    from unimm_amd.policy import PolicyObjective
    return PolicyObjective(mode="ratio")


ONES = torch.ones(SHAPE, dtype=torch.int64)
# (message, the keywords as a function of `w`, what else `bind` takes): tests/test_policy_cpu.py, test_policy_kl_cpu.py, test_pref_cpu.py
REFUSALS = [
    ("pass one of them", lambda w: dict(lm_advantage=w["adv"], lm_weight=ONES), {}),
    ("lm_behaviour_logp", lambda w: dict(lm_advantage=w["adv"], lm_objective=_ratio()), {}),
    (r"\[B, T\]", lambda w: dict(lm_advantage=w["adv"].reshape(-1)), {}),
    (r"\[B, T\]", lambda w: dict(lm_advantage=w["adv"][:, :-1]), {}),
    (r"\[B, T\]", lambda w: dict(lm_advantage=w["adv"], lm_behaviour_logp=w["adv"][:1], lm_objective=_ratio()), {}),
    ("PolicyObjective", lambda w: dict(lm_advantage=w["adv"], lm_objective="logp"), {}),
    ("pass lm_advantage", lambda w: dict(lm_behaviour_logp=w["adv"]), {}),
    ("pass lm_advantage", lambda w: dict(lm_objective=w["kl"]), {}),
    ("computes no loss", lambda w: dict(lm_advantage=w["adv"]), dict(train_branch=False)),
    ("bf16 engine only", lambda w: dict(lm_advantage=w["adv"]), dict(model="fp32x3")),
    # the KL leash
    ("pass lm_reference", lambda w: dict(lm_advantage=w["adv"], lm_objective=w["kl"]), {}),
    ("pass lm_advantage", lambda w: dict(lm_reference=w["ref"]), {}),
    ("pass lm_advantage", lambda w: dict(lm_reference=w["ref"], lm_weight=ONES), {}),
    ("frozen_reference", lambda w: dict(lm_advantage=w["adv"], lm_reference=w["model"]), {}),          # ... also with kl_coef == 0
    # the preference
    ("lm_advantage", lambda w: dict(lm_preference=w["tg"], lm_objective=w["pref"], lm_advantage=w["adv"]), {}),
    ("lm_weight", lambda w: dict(lm_preference=w["tg"], lm_objective=w["pref"], lm_weight=ONES), {}),
    ("lm_behaviour_logp", lambda w: dict(lm_preference=w["tg"], lm_objective=w["pref"], lm_behaviour_logp=w["adv"]), {}),
    ("PreferenceObjective", lambda w: dict(lm_preference=w["tg"]), {}),
    ("PreferenceObjective", lambda w: dict(lm_preference=w["tg"], lm_objective=w["kl"]), {}),
    ("pass lm_advantage", lambda w: dict(lm_objective=w["pref"]), {}),
    ("PreferenceTargets", lambda w: dict(lm_preference=([0, 0], [1.0, 0.0]), lm_objective=w["pref"]), {}),
    ("one of each per sequence", lambda w: dict(lm_preference=_targets([0], [1.0]), lm_objective=w["pref"]), {}),
    ("one of each per", lambda w: dict(lm_preference=_targets([0, 0, 1], [1.0, 0.0, 1.0]), lm_objective=w["pref"]), {}),
    ("finite and >= 0", lambda w: dict(lm_preference=_targets([0, 0], [1.0, -0.5]), lm_objective=w["pref"]), {}),
    ("finite and >= 0", lambda w: dict(lm_preference=_targets([0, 0], [1.0, math.nan]), lm_objective=w["pref"]), {}),
    ("finite and >= 0", lambda w: dict(lm_preference=_targets([0, 0], [1.0, math.inf]), lm_objective=w["pref"]), {}),
    ("group id", lambda w: dict(lm_preference=_targets([0, -1], [1.0, 0.0]), lm_objective=w["pref"]), {}),
    ("beta", lambda w: dict(lm_preference=w["tg"], lm_objective=_broken_beta()), {}),
    ("train branch", lambda w: dict(lm_preference=w["tg"], lm_objective=w["pref"]), dict(train_branch=False)),
    ("bf16 engine only", lambda w: dict(lm_preference=w["tg"], lm_objective=w["pref"]), dict(model="fp32x3")),
    # (a group of more than 128 sequences needs more than two of them: the one case on another shape)
    ("at most 128", lambda w: dict(lm_preference=_targets([0] * 129 + [1], [1.0] * 130), lm_objective=w["pref"]), dict(shape=(130, T))),
]
# every refusal of a reference, under both objectives that read one
REFERENCES = [
    ("frozen_reference", lambda w: w["model"]),
    ("vocab_size", lambda w: _make(vocab_size=w["small"].vocab_size + 8)),
    ("intermediate_size", lambda w: _make(intermediate_size=w["small"].intermediate_size * 2)),
    ("fixed_t_layer", lambda w: _make(fixed_t_layer=1)),
    ("bf16 engine", lambda w: _make("fp32x3")),
    ("is on meta", lambda w: _frozen(w["model"]).to("meta")),
    ("must be a BertForMultiModalPreTraining", lambda w: "checkpoint.bin"),
]
for _msg, _ref in REFERENCES:
    REFUSALS.append((_msg, lambda w, r=_ref: dict(lm_advantage=w["adv"], lm_objective=w["kl"], lm_reference=r(w)), {}))
    REFUSALS.append((_msg, lambda w, r=_ref: dict(lm_preference=w["tg"], lm_objective=w["pref"], lm_reference=r(w)), {}))


@pytest.mark.parametrize("msg,kw,more", REFUSALS, ids=[f"{i}-{c[0]}" for i, c in enumerate(REFUSALS)])
def test_refusal(w, msg, kw, more):
    more = dict(more)
    if more.get("model") == "fp32x3":
        more["model"] = _make("fp32x3")
    with pytest.raises(ValueError, match=msg):
        bind(w, **more, **kw(w))


def test_a_bound_objective_is_the_graph_executors_one_refusal(w):
    """A step whose inputs the executor would replay (every tensor resident) runs eagerly as soon as `inp` carries a bound
    objective, whichever it is -- and only then."""
    from unimm_amd.graphs import _TENSOR_KEYS, StepGraphs
    from unimm_amd.lm_objective import KEY

    class Resident(torch.Tensor):               # a host tensor that says it lives on the device
        is_cuda = property(lambda self: True)

    eng = type("E", (), dict(text_priority=False, cfg=type("Cfg", (), dict(predict_feature=False))()))()
    sg = StepGraphs.__new__(StepGraphs)
    sg.eng = eng
    inp = {k: torch.zeros(1).as_subclass(Resident) for k in _TENSOR_KEYS}
    opts = dict(want_seq=False)
    assert sg.eligible(inp, opts) is True
    for o in (bind(w, lm_advantage=w["adv"]), bind(w, lm_advantage=w["adv"], lm_objective=w["kl"], lm_reference=w["ref"]),
              bind(w, lm_preference=w["tg"], lm_objective=w["pref"])):
        assert sg.eligible({**inp, KEY: o}, opts) is False
    assert sg.eligible({**inp, KEY: None}, opts) is True
