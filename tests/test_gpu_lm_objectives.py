"""Which loss-row entry points one `forward_backward` launches, and in which order, for every objective of the LM head
(unimm_amd/lm_objective.py) on both schedules: the small configuration and the 3 dialogs x 3 answers of
tests/test_gpu_policy_kl_model.py, `unimm_amd.lib._call` wrapped to record the names.  The expected lists below were read off
the engine as it was BEFORE the objectives were bound into one object (the four-way chains of `_lm_head`, `_losses`,
`_lm_loss_grad` and `train_shared`), not off the code under test:

  * a step with a reference starts with the reference's own inference forward, whose head runs the likelihood rows
    (`unimm_lm_loss_fwd`) on the reference's logits before handing them over;
  * the replicated step also computes the image loss, whose `unimm_reduce_sum` follows the LM objective's reductions (the
    shared-context step trains the LM term alone);
  * the fp32x3 engine replaces the likelihood backward by `unimm_x3_lm_loss_bwd`.

Each case also checks that the LM loss is finite and the gradient arena non-zero."""
import pytest
import torch

from tests.test_gpu_policy_kl_model import N_ANSWERS, advantages, perturbed, run
from tests.test_gpu_policy_model import fresh
from tests.test_gpu_shared_training import sampled

pytestmark = pytest.mark.gpu

LOSS_ROWS = {"unimm_lm_loss_fwd", "unimm_lm_loss_bwd", "unimm_x3_lm_loss_bwd", "unimm_pg_loss_fwd", "unimm_pg_loss_bwd",
             "unimm_pg_kl_loss_fwd", "unimm_pg_kl_loss_bwd", "unimm_seq_pref", "unimm_reduce_sum"}

# (objective, schedule, engine) -> the recorded names, filtered to LOSS_ROWS
EXPECTED = {
    ("likelihood", "replicated", "bf16"): [
        "unimm_lm_loss_fwd", "unimm_reduce_sum", "unimm_reduce_sum", "unimm_lm_loss_bwd"],             # loss; image loss
    ("likelihood", "shared", "bf16"): [
        "unimm_lm_loss_fwd", "unimm_reduce_sum", "unimm_lm_loss_bwd"],
    ("likelihood", "replicated", "fp32x3"): [
        "unimm_lm_loss_fwd", "unimm_reduce_sum", "unimm_reduce_sum", "unimm_x3_lm_loss_bwd"],
    ("policy", "replicated", "bf16"): [
        "unimm_pg_loss_fwd", "unimm_reduce_sum", "unimm_reduce_sum", "unimm_reduce_sum", "unimm_pg_loss_bwd"],   # loss, entropy; image
    ("policy", "shared", "bf16"): [
        "unimm_pg_loss_fwd", "unimm_reduce_sum", "unimm_reduce_sum", "unimm_pg_loss_bwd"],
    ("policy_kl", "replicated", "bf16"): [
        "unimm_lm_loss_fwd",                                                                           # the reference's forward
        "unimm_pg_kl_loss_fwd", "unimm_reduce_sum", "unimm_reduce_sum", "unimm_reduce_sum", "unimm_reduce_sum",  # loss, entropy, KL; image
        "unimm_pg_kl_loss_bwd"],
    ("policy_kl", "shared", "bf16"): [
        "unimm_lm_loss_fwd",
        "unimm_pg_kl_loss_fwd", "unimm_reduce_sum", "unimm_reduce_sum", "unimm_reduce_sum", "unimm_pg_kl_loss_bwd"],
    ("preference", "replicated", "bf16"): [
        "unimm_lm_loss_fwd", "unimm_seq_pref", "unimm_reduce_sum", "unimm_reduce_sum", "unimm_pg_loss_bwd"],
    ("preference", "shared", "bf16"): [
        "unimm_lm_loss_fwd", "unimm_seq_pref", "unimm_reduce_sum", "unimm_pg_loss_bwd"],
    ("preference_ref", "replicated", "bf16"): [
        "unimm_lm_loss_fwd",                                                                           # the reference's forward
        "unimm_lm_loss_fwd", "unimm_lm_loss_fwd", "unimm_seq_pref",                                    # the policy's rows, the reference's
        "unimm_reduce_sum", "unimm_reduce_sum", "unimm_pg_loss_bwd"],
    ("preference_ref", "shared", "bf16"): [
        "unimm_lm_loss_fwd",
        "unimm_lm_loss_fwd", "unimm_lm_loss_fwd", "unimm_seq_pref", "unimm_reduce_sum", "unimm_pg_loss_bwd"],
}


@pytest.fixture(scope="module")
def world():
    """one model per engine, a perturbed frozen copy of the bf16 one, 3 dialogs x 3 answers"""
    model = fresh()
    d, sb = sampled(N_ANSWERS)
    return dict(bf16=model, fp32x3=fresh("fp32x3"), ref=perturbed(model), d=d, sb=sb)


def objective_kw(name, world):
    from unimm_amd.policy import PolicyObjective, PreferenceObjective, PreferenceTargets
    sb = world["sb"]
    if name == "likelihood":
        return {}
    if name == "policy":
        return dict(lm_advantage=advantages(sb), lm_objective=PolicyObjective(entropy_coef=0.01))
    if name == "policy_kl":
        return dict(lm_advantage=advantages(sb), lm_objective=PolicyObjective(entropy_coef=0.01, kl_coef=0.5), lm_reference=world["ref"])
    weight = torch.rand(sb.input_ids.shape[0], generator=torch.Generator().manual_seed(4))
    kw = dict(lm_preference=PreferenceTargets(sb.image_index, weight), lm_objective=PreferenceObjective(0.5, True))
    return dict(kw, lm_reference=world["ref"]) if name == "preference_ref" else kw


@pytest.mark.parametrize("objective,schedule,engine", list(EXPECTED), ids=["-".join(k) for k in EXPECTED])
def test_loss_row_launches(world, monkeypatch, objective, schedule, engine):
    from unimm_amd import lib as L
    names, inner = [], L._call

    def recording(name, *args):
        names.append(name)
        return inner(name, *args)

    model = world[engine]
    model.engine.ensure(torch.device("cuda", 0))
    kw = objective_kw(objective, world)
    monkeypatch.setattr(L, "_call", recording)
    lm_loss, grads = run(model, world["d"], world["sb"], shared=schedule == "shared", **kw)
    monkeypatch.undo()
    assert [n for n in names if n in LOSS_ROWS] == EXPECTED[objective, schedule, engine]
    assert bool(torch.isfinite(lm_loss).all()) and float(grads.abs().max()) > 0
