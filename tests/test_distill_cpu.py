"""Knowledge distillation on the host: the float64 restatement (tests/distill_ref.py) against autograd, the fp32 restatement of
the forward in the kernel's operation order against the error budgets of tests/test_gpu_distill_edges.py, and every refusal of
`policy.bind_objective` and of the teacher check.  Nothing here loads the library or touches a device."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import distill_ref as DR
from tests import test_gpu_distill_edges as DE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = B, T = 2, 16


# ---- the float64 reference against autograd ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0, 4.0])
@pytest.mark.parametrize("alpha", [0.0, 0.3, 1.0])
def test_reference_matches_autograd(tau, alpha):
    rng = np.random.default_rng(int(tau * 10 + alpha * 100))
    n, V = 12, 57
    z = rng.standard_normal((n, V)) * 2
    zr = rng.standard_normal((n, V)) * 2
    y = rng.integers(0, V, n)
    w = np.array([(1, 3, -1, 0)[i % 4] for i in range(n)])
    y[5], y[10] = -1, -1                                            # a likelihood row and an unlikelihood row without a label
    z[2, y[2]] = 25.0                                               # an unlikelihood row past the clamp: a zero hard gradient
    fw = DR.forward(z, zr, y, w, tau, alpha)
    grad = DR.backward(fw, y, w, 1.0)[0]
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    zrt = torch.tensor(zr, dtype=torch.float64, requires_grad=True)
    total = DR.torch_objective(zt, zrt, y, w, tau, alpha)
    gz, gzr = torch.autograd.grad(total, (zt, zrt), allow_unused=True)
    assert abs(float(total.detach()) - fw["rowloss"].sum()) <= 1e-12 * max(1.0, abs(float(total.detach())))
    assert np.abs(gz.numpy() - grad).max() <= 1e-12
    assert gzr is None or float(gzr.abs().max()) == 0.0             # nothing flows into the teacher
    off = ~fw["part"]
    assert off.sum() == 5 and (fw["rowloss"][off] == 0).all() and (fw["kd"][off] == 0).all() and (grad[off] == 0).all()
    assert 1.0 - fw["py"][2] < DR.CLAMP and (alpha == 0 or (DR.backward(fw, y, w, 1.0)[1][2] == 0).all())
    if alpha < 1:
        assert (fw["kd"][fw["part"]] > 0).all()


def test_reference_with_minus_infinity():
    """q_i = 0 contributes exactly 0 whatever z_i holds; the teacher equal to the student gives KD = 0 and no soft gradient"""
    z = np.array([[1.0, -np.inf, 0.5, 2.0], [0.0, 1.0, -np.inf, -np.inf]])
    zr = np.array([[0.5, -np.inf, -np.inf, 1.0], [0.3, 0.2, -np.inf, -np.inf]])
    y, w = np.array([0, 1]), np.array([1, -1])
    fw = DR.forward(z, zr, y, w, 2.0, 0.5)
    g = DR.backward(fw, y, w, 1.0)[0]
    assert np.isfinite(fw["kd"]).all() and np.isfinite(fw["rowloss"]).all() and np.isfinite(g).all()
    assert g[0, 1] == 0 and (g[1, 2:] == 0).all() and g[0, 2] > 0   # p_2 > 0 = q_2: the student's own share
    same = DR.forward(z, z, y, w, 2.0, 0.0)
    assert (same["kd"] == 0).all() and (DR.backward(same, y, w, 1.0)[0] == 0).all()


# ---- the fp32 restatement of the forward inside the error budgets --------------------------------------------------------------
@pytest.mark.parametrize("V,ld,ld_ref", [(30522, 30528, 30528), (4100, 4100, 4100), (1000, 1001, 1000), (8, 8, 8), (3, 4, 3)])
def test_fp32_forward_stays_inside_the_error_budgets(V, ld, ld_ref):
    kinds, z, zr, y, w, rk = DE.rows(V, ld, ld_ref)
    gated = np.arange(len(y)) != DE.OUTSIDE
    for tau in DE.TAUS + (4.0, 3.0):                                # (3: a temperature whose reciprocal is rounded)
        fw = DR.forward(z[:, :V], zr[:, :V], y, w, tau, 0.0)
        al = DR.allowances(fw, z[:, :V], zr[:, :V], y, w, 1.0)
        lse, lse_t, rlse_t, kd = (v.astype(np.float64) for v in DR.forward_f32(z[:, :V], zr[:, :V], tau, vec=ld % 4 == 0))
        assert not np.isnan(np.stack([lse, lse_t, rlse_t, kd])[:, gated]).any()
        worst = {}
        for name, got, ref, allow in (("lse", lse, fw["lse"], al["A"]), ("lse_t", lse_t, fw["lse_t"], al["At"]),
                                      ("ref_lse_t", rlse_t, fw["ref_lse_t"], al["Art"]), ("kd", kd, fw["kd_raw"], al["EKD"])):
            ratio = (np.abs(got - ref) / allow)[gated]
            worst[name] = float(ratio.max())
            assert (ratio <= 1.0).all(), (name, V, tau, int(np.argmax(ratio)), worst[name])
        print(f"[distill-cpu] fp32 forward V={V} ld={ld} tau={tau}: worst error / allowance " +
              ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        if tau == 1.0:
            assert (lse_t == lse).all()                             # the same operations on the same numbers
        same = DR.forward_f32(z[:, :V], z[:, :V], tau, vec=ld % 4 == 0)
        assert (same[3] == 0).all() and (same[2] == same[1]).all()  # the teacher's sums take the student's sequence


# ---- bind_objective ------------------------------------------------------------------------------------------------------------
def _make(dtype="bf16", **over):
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json")))
    cfg.update(over)
    return BertForMultiModalPreTraining(BertConfig.from_dict(cfg), compute_dtype=dtype)


@pytest.fixture(scope="module")
def w():
    from unimm_amd.policy import DistillObjective, PreferenceTargets, frozen_reference
    torch.manual_seed(0)
    model = _make()
    teacher = _make(num_hidden_layers=2, t_biattention_id=[0, 1])
    teacher.eval()
    teacher.requires_grad_(False)
    return dict(model=model, teacher=teacher, frozen=frozen_reference(model), obj=DistillObjective(), adv=torch.zeros(SHAPE),
                tg=PreferenceTargets([0, 0], [1.0, 0.0]), small=model.config)


def bind(w, train_branch=True, model=None, **kw):
    from unimm_amd.policy import bind_objective
    return bind_objective(w["model"] if model is None else model, SHAPE, train_branch, **kw)


def test_the_objective_is_a_validated_frozen_dataclass():
    import dataclasses
    import unimm_amd
    from unimm_amd.policy import DistillObjective
    assert unimm_amd.DistillObjective is DistillObjective and "DistillObjective" in unimm_amd.__all__
    o = DistillObjective()
    assert (o.temperature, o.alpha) == (2.0, 0.5) and DistillObjective(4.0, 0.0) == DistillObjective(temperature=4.0, alpha=0.0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.alpha = 0.1
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.inf), dict(temperature=math.nan),
               dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=math.nan), dict(alpha="half")):
        with pytest.raises(ValueError, match="DistillObjective"):
            DistillObjective(**kw)


def test_a_teacher_of_another_depth_binds(w):
    from unimm_amd.lm_objective import REPORTS, Distillation
    from unimm_amd.policy import DistillObjective
    assert w["teacher"].config.num_hidden_layers != w["model"].config.num_hidden_layers
    o = bind(w, lm_objective=w["obj"], lm_reference=w["teacher"])
    assert type(o) is Distillation and o.reference is w["teacher"] and o.ref is None and (o.tau, o.alpha) == (2.0, 0.5)
    for member in ("stage", "forward", "loss", "backward", "reference"):
        assert hasattr(o, member)
    assert "last_lm_distill" in REPORTS and w["model"].engine.last_lm_distill is None
    # lm_weight means what it means to the likelihood; a frozen copy serves self-distillation; either model class may teach
    ones = torch.ones(SHAPE, dtype=torch.int64)
    assert type(bind(w, lm_objective=w["obj"], lm_reference=w["teacher"], lm_weight=ones)) is Distillation
    assert bind(w, lm_objective=DistillObjective(1.0, 0.0), lm_reference=w["frozen"]).reference is w["frozen"]
    # wider, with other heads and another schedule
    wide = _make(hidden_size=192, num_attention_heads=3, intermediate_size=512, v_hidden_size=128, bi_hidden_size=128,
                 with_coattention=False, fixed_t_layer=1, v_target_size=w["small"].v_target_size)
    assert bind(w, lm_objective=w["obj"], lm_reference=wide).reference is wide
    # alpha == 1 reads nothing of the teacher: it is judged, and its forward does not run
    assert bind(w, lm_objective=DistillObjective(alpha=1.0), lm_reference=w["teacher"]).reference is None


def test_the_graph_executor_declines_it(w):
    from unimm_amd.graphs import _TENSOR_KEYS, StepGraphs
    from unimm_amd.lm_objective import KEY

    class Resident(torch.Tensor):
        is_cuda = property(lambda self: True)

    sg = StepGraphs.__new__(StepGraphs)
    sg.eng = type("E", (), dict(text_priority=False, cfg=type("Cfg", (), dict(predict_feature=False))()))()
    inp = {k: torch.zeros(1).as_subclass(Resident) for k in _TENSOR_KEYS}
    assert sg.eligible(inp, dict(want_seq=False)) is True
    assert sg.eligible({**inp, KEY: bind(w, lm_objective=w["obj"], lm_reference=w["teacher"])}, dict(want_seq=False)) is False


def _broken(**kw):
    from unimm_amd.policy import DistillObjective
    o = DistillObjective()
    for k, v in kw.items():
        object.__setattr__(o, k, v)                                 # past the constructor's own check
    return o


REFUSALS = [
    ("pass the teacher as lm_reference", lambda w: dict(lm_objective=w["obj"]), {}),
    ("pass the teacher as lm_reference", lambda w: dict(lm_objective=w["obj"], lm_weight=torch.ones(SHAPE, dtype=torch.int64)), {}),
    ("lm_advantage", lambda w: dict(lm_objective=w["obj"], lm_reference=w["teacher"], lm_advantage=w["adv"]), {}),
    ("lm_behaviour_logp", lambda w: dict(lm_objective=w["obj"], lm_reference=w["teacher"], lm_behaviour_logp=w["adv"]), {}),
    ("lm_preference", lambda w: dict(lm_objective=w["obj"], lm_reference=w["teacher"], lm_preference=w["tg"]), {}),
    ("bf16 engine only", lambda w: dict(lm_objective=w["obj"], lm_reference=w["teacher"]), dict(model="fp32x3")),
    ("computes no loss", lambda w: dict(lm_objective=w["obj"], lm_reference=w["teacher"]), dict(train_branch=False)),
    ("temperature", lambda w: dict(lm_objective=_broken(temperature=0.0), lm_reference=w["teacher"]), {}),
    ("alpha", lambda w: dict(lm_objective=_broken(alpha=2.0), lm_reference=w["teacher"]), {}),
    # the teacher
    ("trained model itself", lambda w: dict(lm_objective=w["obj"], lm_reference=w["model"]), {}),
    ("must be a BertForMultiModalPreTraining", lambda w: dict(lm_objective=w["obj"], lm_reference="teacher.bin"), {}),
    ("is on meta", lambda w: dict(lm_objective=w["obj"], lm_reference=_make(num_hidden_layers=2, t_biattention_id=[0, 1]).to("meta")), {}),
    ("bf16 engine", lambda w: dict(lm_objective=w["obj"], lm_reference=_make("fp32x3")), {}),
    ("vocab_size", lambda w: dict(lm_objective=w["obj"], lm_reference=_make(vocab_size=w["small"].vocab_size + 8)), {}),
    ("v_feature_size", lambda w: dict(lm_objective=w["obj"], lm_reference=_make(v_feature_size=w["small"].v_feature_size * 2)), {}),
    ("type_vocab_size", lambda w: dict(lm_objective=w["obj"], lm_reference=_make(type_vocab_size=3)), {}),
    ("max_position_embeddings", lambda w: dict(lm_objective=w["obj"], lm_reference=_make(max_position_embeddings=256)), {}),
    # ... and alpha == 1 does not excuse a teacher that is none
    ("trained model itself", lambda w: dict(lm_objective=_broken(alpha=1.0), lm_reference=w["model"]), {}),
]


@pytest.mark.parametrize("msg,kw,more", REFUSALS, ids=[f"{i}-{c[0]}" for i, c in enumerate(REFUSALS)])
def test_refusal(w, msg, kw, more):
    more = dict(more)
    if more.get("model") == "fp32x3":
        more["model"] = _make("fp32x3")
    with pytest.raises(ValueError, match=msg):
        bind(w, **more, **kw(w))


def test_the_existing_checks_keep_their_words(w):
    """a reference alone, or with lm_weight, still asks for lm_advantage; check_reference still insists on the trained model's
    shape under the two objectives that had a reference before"""
    from unimm_amd.policy import PolicyObjective, PreferenceObjective
    with pytest.raises(ValueError, match="pass lm_advantage"):
        bind(w, lm_reference=w["teacher"])
    with pytest.raises(ValueError, match="pass lm_advantage"):
        bind(w, lm_reference=w["teacher"], lm_weight=torch.ones(SHAPE, dtype=torch.int64))
    with pytest.raises(ValueError, match="num_hidden_layers"):
        bind(w, lm_advantage=w["adv"], lm_objective=PolicyObjective(kl_coef=0.5), lm_reference=w["teacher"])
    with pytest.raises(ValueError, match="num_hidden_layers"):
        bind(w, lm_preference=w["tg"], lm_objective=PreferenceObjective(), lm_reference=w["teacher"])
    with pytest.raises(ValueError, match="PolicyObjective"):
        bind(w, lm_advantage=w["adv"], lm_objective="distill")


def test_the_harness_passes_model_keywords_through_and_nothing_else():
    """harness.forward(model_kw=...) hands the keywords to the encoder's call; without them the call is today's"""
    from unimm_amd import harness
    seen = []

    def encoder(tokens, feat, loc, **kw):
        seen.append(kw)
        one = torch.ones(1)
        return one, one, one

    n, T_, R = 3, 4, 2
    batch = dict(tokens=torch.zeros((1, n, T_), dtype=torch.int64), sep_indices=torch.zeros((1, n, 2), dtype=torch.int64),
                 hist_len=torch.zeros((1, n), dtype=torch.int64), segments=torch.zeros((1, n, T_), dtype=torch.int64),
                 positions=torch.zeros((1, n, T_), dtype=torch.int64), mask=torch.zeros((1, n, T_), dtype=torch.int64),
                 txt_attention_mask=torch.zeros((1, n, T_, T_)), co_attention_mask=torch.zeros((1, n, R, T_)),
                 image_mask=torch.zeros((1, n, R)), weights=torch.ones((1, n, T_), dtype=torch.int64),
                 next_sentence_labels=torch.zeros((1, n), dtype=torch.int64), image_target=torch.zeros((1, n, R, 5)),
                 image_label=torch.zeros((1, n, R), dtype=torch.int64), image_feat=torch.zeros((1, n, R, 6)),
                 image_loc=torch.zeros((1, n, R, 5)))
    params = dict(lm_loss_coeff=1.0, nsp_loss_coeff=1.0, img_loss_coeff=1.0)
    harness.forward(encoder, batch, params)
    harness.forward(encoder, batch, params, model_kw=dict(lm_objective="o", lm_reference="t"))
    assert "lm_objective" not in seen[0] and "lm_reference" not in seen[0]
    assert seen[1]["lm_objective"] == "o" and seen[1]["lm_reference"] == "t"
    assert set(seen[1]) - set(seen[0]) == {"lm_objective", "lm_reference"} and "lm_weight" in seen[0]
