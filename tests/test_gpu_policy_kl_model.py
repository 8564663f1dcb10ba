"""The KL leash of the policy-gradient step (PolicyObjective.kl_coef + lm_reference) through the engine, the model surface and
trainer.self_critical_step, on the small configuration, T = 64, 3 dialogs x 3 sampled answers: kl_coef = 0 with a reference
against the step without one (bit for bit), the kernels on the model's own rows against the float64 restatement with the
allowances of tests/test_gpu_policy_kl_edges.py, the wiring (a copy of the model is at KL ~ 0, a perturbed copy is not), the
direction of one gradient step, the shared schedule against the replicated one, the loop body, the refusals on the device."""
import math

import numpy as np
import pytest
import torch

from tests import policy_kl_ref as KR
from tests import policy_ref as PR
from tests import test_gpu_policy_edges as PE
from tests.test_gpu_policy_kl_edges import U, gate, grad_ratio, kl_allowances
from tests.test_gpu_policy_model import MAXLEN, _encoder, fresh, policy_inputs, tiny_dialogs
from tests.test_gpu_shared_training import LOSS_TOL, sampled

pytestmark = pytest.mark.gpu
N_ANSWERS = 3


def perturbed(model, seed=17):
    """a frozen copy of the model with seeded noise on its decoder bias and one text layer"""
    from unimm_amd.policy import frozen_reference
    ref = frozen_reference(model)
    gen = torch.Generator().manual_seed(seed)
    sd = dict(ref.named_parameters())
    with torch.no_grad():
        for name, sigma in (("cls.predictions.bias", 0.5), ("bert.encoder.layer.1.output.dense.weight", 0.02)):
            p = sd[name]
            p.add_((torch.randn(p.shape, generator=gen) * sigma).to(p.device))
    ref.engine.invalidate_weights()
    return ref


def snapshot(ref):
    return {k: v.detach().clone() for k, v in ref.state_dict().items()}, ref.engine.step, ref.engine.seed, ref.training


def assert_untouched(ref, snap):
    sd, step, seed, training = snap
    now = ref.state_dict()
    assert sd.keys() == now.keys()
    for k, v in sd.items():
        assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v,
                           now[k].view(torch.int32) if v.dtype == torch.float32 else now[k]), k
    assert all(p.grad is None and not p.requires_grad for p in ref.parameters())
    assert (ref.engine.step, ref.engine.seed, ref.training) == (step, seed, training)


def run(model, d, sb, *, shared=False, train=True, seed=9, **more):
    """one forward_backward from zeroed gradients under a fixed dropout seed and step -> (LM loss, gradient arena)"""
    from unimm_amd import SharedContext
    model.train(train)
    model.engine.ensure(torch.device("cuda", 0))
    model.set_dropout_seed(seed, 0)
    model.engine.arena.zero_grads()
    model.engine.last_lm_kl = None
    kw = policy_inputs(sb, d, d["image_feat"].shape[0], model.config.v_target_size)
    kw.update(more)
    if shared:
        kw["shared_context"] = SharedContext(sb.image_index, 64)
    res = model.forward_backward(sb.input_ids, d["image_feat"], d["image_loc"], (1.0, 0.0, 0.0), **kw)
    torch.cuda.synchronize()
    return res[1].clone(), model.engine.arena.grad_flat.clone()


def advantages(sb, seed=2, zero=False):
    from unimm_amd.policy import spread
    G, N = sb.shape
    adv = torch.randn((G, N), generator=torch.Generator().manual_seed(seed))
    return spread(torch.zeros_like(adv) if zero else adv, sb)


class Spy:
    """records what `_lm_loss_grad` reads and returns"""

    def __init__(self, model):
        self.engine, self.inner, self.calls = model.engine, model.engine._lm_loss_grad, []
        model.engine._lm_loss_grad = self

    def __call__(self, lm, g_lm):
        pg = lm["objective"]                   # the step's bound lm_objective.PolicyGradient
        rec = dict(logits=lm["logits"].clone(), ref=None if pg.ref is None else pg.ref.clone(), labels=lm["labels"].clone(),
                   adv=pg.adv[pg.pos.long()].clone(), n=lm["n"], g=float(g_lm.reshape(-1)[0]),
                   inv=float(lm["inv_dev"][0]) if lm.get("inv_dev") is not None else 1.0 / lm["n"],
                   **{k: None if lm.get(k) is None else lm[k].clone() for k in ("kl", "ref_lse", "rowloss", "lse", "ent")})
        rec["dlog"] = self.inner(lm, g_lm).clone()
        rec["released"] = pg.ref is None
        self.calls.append(rec)
        return rec["dlog"]

    def close(self):
        self.engine._lm_loss_grad = self.inner


@pytest.fixture(scope="module")
def world():
    """one model, its perturbed and its identical frozen copy, 3 dialogs x 3 answers"""
    from unimm_amd.policy import frozen_reference
    model = fresh()
    d, sb = sampled(N_ANSWERS)
    return dict(model=model, far=perturbed(model), same=frozen_reference(model), d=d, sb=sb)


def test_kl_coef_zero_with_a_reference_is_todays_step(world):
    """PolicyObjective(kl_coef=0) with lm_reference given: accepted and ignored.  Same dropout seed and step as the step without
    a reference: the LM loss and the LM head's gradient bit for bit; the gradient arena bit for bit on the shared schedule (whose
    embedding gradient is added in a fixed order) and, on the replicated schedule, on every bucket on which three runs WITHOUT a
    reference agree among themselves (the word-embedding rows collect fp32 atomics there, tests/test_gpu_policy_model.py: a
    bucket that does not repeat is held to 2x the spread of those three runs).  The reference is not touched, and no reference
    forward runs."""
    from unimm_amd.policy import PolicyObjective
    model, ref, d, sb = world["model"], world["far"], world["d"], world["sb"]
    snap = snapshot(ref)
    ran = []
    inner = ref.engine.forward
    ref.engine.forward = lambda *a, **k: ran.append(1) or inner(*a, **k)
    obj = PolicyObjective(entropy_coef=0.01, kl_coef=0.0)
    more = dict(lm_advantage=advantages(sb), lm_objective=obj)
    spy = Spy(model)
    try:
        for shared in (True, False):
            old = [run(model, d, sb, shared=shared, **more) for _ in range(3)]
            new = run(model, d, sb, shared=shared, lm_reference=ref, **more)
            assert model.engine.last_lm_kl is None and model.engine.last_lm_entropy is not None
            assert torch.equal(new[0].view(torch.int32), old[0][0].view(torch.int32)) and bool(torch.isfinite(new[0]).all())
            heads = spy.calls[-4:]
            assert all(torch.equal(h["dlog"].view(torch.int16), heads[0]["dlog"].view(torch.int16)) for h in heads)
            assert heads[3]["ref"] is None and heads[3]["kl"] is None and bool((heads[3]["dlog"] != 0).any())
            noisy = 0
            for name, lo, hi in model.engine.arena.used_ranges():
                o = [r[1][lo:hi] for r in old]
                spread = max(float((o[i] - o[j]).abs().max()) for i, j in ((0, 1), (0, 2), (1, 2)))
                if spread == 0.0:
                    assert torch.equal(new[1][lo:hi].view(torch.int32), o[0].view(torch.int32)), (shared, name)
                else:
                    noisy += 1
                    assert float((new[1][lo:hi] - o[0]).abs().max()) <= 2 * spread, (shared, name)
            print(f"\nshared = {shared}: {len(model.engine.arena.used_ranges()) - noisy} buckets bit-equal, {noisy} not reproducible "
                  "in the step without a reference itself")
            assert noisy == 0 if shared else noisy < len(model.engine.arena.used_ranges())
            assert float(new[1].abs().max()) > 0
    finally:
        spy.close()
        del ref.engine.forward                 # (the instance attribute: the class's method is back)
    assert not ran, "kl_coef = 0: no second forward"
    assert_untouched(ref, snap)


def test_kernels_on_the_models_own_rows(world):
    """The policy's and the reference's logits rows of one train-mode step, as `_lm_loss_grad` reads them: kl, rowloss and the
    bf16 gradient matrix against the float64 restatement with the allowances of tests/test_gpu_policy_kl_edges.py;
    engine.last_lm_kl = the mean of those rows' kl within n U max|kl| (a sum of n fp32 numbers and one product)."""
    from unimm_amd.policy import PolicyObjective
    model, ref, d, sb = world["model"], world["far"], world["d"], world["sb"]
    snap = snapshot(ref)
    beta, kl_coef = 0.01, 0.5
    spy = Spy(model)
    try:
        lm_loss, _ = run(model, d, sb, lm_advantage=advantages(sb), lm_reference=ref,
                         lm_objective=PolicyObjective(entropy_coef=beta, kl_coef=kl_coef))
    finally:
        spy.close()
    rec = spy.calls[-1]
    V, n = model.config.vocab_size, rec["n"]
    assert n == int((sb.masked_lm_labels != -1).sum()) and rec["ref"].shape == rec["logits"].shape and rec["released"]
    assert rec["ref"].data_ptr() != rec["logits"].data_ptr() and not torch.equal(rec["ref"], rec["logits"])
    z, zr = rec["logits"][:, :V].cpu().numpy(), rec["ref"][:, :V].cpu().numpy()
    y, adv = rec["labels"].cpu().numpy(), rec["adv"].cpu().numpy()
    assert (y >= 0).all() and np.isfinite(z).all() and np.isfinite(zr).all()
    gs = float(np.float32(rec["g"]) * np.float32(rec["inv"]))
    assert abs(rec["inv"] - 1.0 / n) <= 1e-6 / n
    fw = KR.forward(z, zr, y, adv, None, PR.LOGP, math.inf, beta, kl_coef)
    grad_r = KR.backward(fw, y, beta, gs)[0]
    a64 = adv.astype(np.float64)
    al = PE.allowances(fw, gs, beta, PR.LOGP, a64, np.zeros(n), y)
    ka = kl_allowances(fw, al, gs, kl_coef)
    got_kl = rec["kl"].double().cpu().numpy()
    gate("(model rows) kl (abs / E_KL)", np.abs(got_kl - fw["kl"]) / ka["EKL"], 1.0)
    gate("(model rows) ref_lse (abs / A)", np.abs(rec["ref_lse"].double().cpu().numpy() - fw["ref_lse"]) / ka["Ar"], 1.0)
    loss_allow = np.abs(a64) * al["A"] + beta * al["EH"] + kl_coef * ka["EKL"] + 1e-6 * np.abs(fw["rowloss"])
    gate("(model rows) rowloss (abs)", np.abs(rec["rowloss"].double().cpu().numpy() - fw["rowloss"]), loss_allow)
    gd = rec["dlog"].float().double().cpu().numpy()
    gate("(model rows) grad (err / allowance)", grad_ratio(gd[:, :V], grad_r, ka["abs_err"]), 1.0)
    assert (gd[:, V:] == 0).all()
    assert fw["kl"].min() > 1e-3, "the perturbed reference is away from the policy on every row"
    mean = float(model.engine.last_lm_kl)
    print(f"\nmean KL of {n} rows: engine {mean:.6f}, restatement {fw['kl'].mean():.6f}; lm_loss {float(lm_loss):.6f}")
    assert abs(mean - float(rec["kl"].double().mean())) <= n * U * float(rec["kl"].abs().max())
    assert abs(float(lm_loss) - fw["rowloss"].mean()) <= loss_allow.mean() + n * U * np.abs(fw["rowloss"]).max()
    assert_untouched(ref, snap)


def eval_kl(model, d, sb, ref, shared=False, kl_coef=1.0):
    """eval-mode step with all advantages zero -> (LM loss = kl_coef x mean KL, mean KL, mean E_KL of the rows)"""
    from unimm_amd.policy import PolicyObjective
    spy = Spy(model)
    try:
        lm_loss, _ = run(model, d, sb, shared=shared, train=False, lm_advantage=advantages(sb, zero=True), lm_reference=ref,
                         lm_objective=PolicyObjective(kl_coef=kl_coef))
    finally:
        spy.close()
    rec = spy.calls[-1]
    V = model.config.vocab_size
    fw = KR.forward(rec["logits"][:, :V].cpu().numpy(), rec["ref"][:, :V].cpu().numpy(), rec["labels"].cpu().numpy(),
                    np.zeros(rec["n"]), None, PR.LOGP, math.inf, 0.0, kl_coef)
    ekl = U * (512 + 6 * np.abs(fw["lse"]) + 6 * np.abs(fw["ref_lse"]) + 518 * fw["adiff"])
    return float(lm_loss), float(model.engine.last_lm_kl), float(ekl.mean())


def test_wiring_a_copy_is_at_zero_a_perturbed_copy_is_not(world):
    """eval mode (the reference runs without dropout): against `frozen_reference(model)` the mean KL is at most 1e-2 of the mean
    KL against the perturbed copy -- rows of another position, another order or another model would not be; both >= -E_KL."""
    model, d, sb = world["model"], world["d"], world["sb"]
    loss_same, kl_same, e_same = eval_kl(model, d, sb, world["same"])
    loss_far, kl_far, e_far = eval_kl(model, d, sb, world["far"])
    print(f"\nmean KL against an identical copy {kl_same:.3e} (E_KL {e_same:.1e}), against the perturbed copy {kl_far:.3e} (E_KL {e_far:.1e})")
    assert kl_same >= -e_same and kl_far >= -e_far
    assert kl_far > 1e-3 and kl_same <= 1e-2 * kl_far
    assert abs(loss_far - kl_far) <= 1e-6 * kl_far + 2 * U                   # all advantages zero, kl_coef = 1: the loss IS the mean KL


KL_LR = 1e-2


def test_the_penalty_pulls_the_policy_towards_the_reference():
    """All advantages zero, kl_coef = 1, perturbed reference, eval mode: one plain step p -= lr grad, and the eval-mode mean KL,
    recomputed by a second call, falls (the pattern of test_one_gradient_step_moves_the_samples_apart)."""
    model = fresh()
    ref = perturbed(model)
    d, sb = sampled(N_ANSWERS)
    snap = snapshot(ref)
    _, before, _ = eval_kl(model, d, sb, ref)
    with torch.no_grad():
        assert float(model.engine.arena.grad_flat.abs().max()) > 0
        model.engine.arena.flat.sub_(KL_LR * model.engine.arena.grad_flat)
    model.engine.invalidate_weights()
    _, after, _ = eval_kl(model, d, sb, ref)
    print(f"\nmean KL to the reference {before:.6f} -> {after:.6f}")
    assert math.isfinite(after) and after < before
    assert_untouched(ref, snap)


def test_shared_and_replicated_schedules_agree(world):
    """eval mode (the two schedules draw their dropout masks at different sites): lm_loss and last_lm_kl of the shared step equal
    the replicated step's within the gate of tests/test_gpu_shared_training.py for shared against replicated."""
    from unimm_amd.policy import PolicyObjective
    model, ref, d, sb = world["model"], world["far"], world["d"], world["sb"]
    got = {}
    for shared in (False, True):
        lm, _ = run(model, d, sb, shared=shared, train=False, lm_advantage=advantages(sb), lm_reference=ref,
                    lm_objective=PolicyObjective(entropy_coef=0.01, kl_coef=0.5))
        got[shared] = (float(lm), float(model.engine.last_lm_kl))
    print(f"\nreplicated lm_loss {got[False][0]:.6f} KL {got[False][1]:.6f}; shared lm_loss {got[True][0]:.6f} KL {got[True][1]:.6f}")
    for i in (0, 1):
        assert math.isfinite(got[True][i]) and abs(got[True][i] - got[False][i]) <= LOSS_TOL * max(abs(got[False][i]), 1e-3)
    assert got[False][1] > 1e-3


@pytest.mark.parametrize("shared", [False, True])
def test_self_critical_step_with_a_reference(shared):
    from unimm_amd import trainer
    from unimm_amd.policy import PolicyObjective, frozen_reference
    enc, opt, sch = _encoder()
    ref = frozen_reference(enc)
    snap = snapshot(ref.bert_pretrained)
    d, c, _ = tiny_dialogs(G=4, seed=8)
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"])
    eng = enc.bert_pretrained.engine
    eng.ensure(torch.device("cuda", 0))
    p0 = eng.arena.flat.clone()
    out = trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), 1, lambda tokens, lengths: -lengths.float(),
                                     samples=3, baseline="mean", objective=PolicyObjective(kl_coef=0.05), max_answer_len=MAXLEN,
                                     seed=4, shared_context=shared, reference=ref)
    torch.cuda.synchronize()
    print(f"\nself_critical_step(reference, shared_context={shared}): {out}, mean KL {float(eng.last_lm_kl):.4e}")
    assert len(out) == 4 and all(math.isfinite(v) for v in out)
    assert eng.last_lm_kl is not None and eng.last_lm_kl.shape == (1,) and eng.last_lm_kl.dtype == torch.float32
    assert math.isfinite(float(eng.last_lm_kl)) and float(eng.last_lm_kl) >= 0     # train mode: dropout moves the policy off its copy
    assert enc.training and not ref.training
    assert not torch.equal(p0, eng.arena.flat), "the optimizer stepped"
    assert torch.isfinite(eng.arena.flat).all()
    assert_untouched(ref.bert_pretrained, snap)


def test_reference_refusals_on_the_device(world):
    import json
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    from unimm_amd.policy import PolicyObjective, frozen_reference
    from tests.test_gpu_policy_model import CFG
    model, d, sb = world["model"], world["d"], world["sb"]
    kw = policy_inputs(sb, d, d["image_feat"].shape[0], model.config.v_target_size)
    kw.update(lm_advantage=advantages(sb), lm_objective=PolicyObjective(kl_coef=0.05))
    cfgd = json.load(open(CFG))
    cfgd["vocab_size"] += 64
    other_vocab = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd)).cuda()
    for ref, msg in ((fresh("fp32x3"), "bf16 engine"), (other_vocab, "vocab_size"), (model, "frozen_reference"),
                     (frozen_reference(model).cpu(), "is on cpu")):
        with pytest.raises(ValueError, match=msg):
            model.forward_backward(sb.input_ids, d["image_feat"], d["image_loc"], (1.0, 0.0, 0.0), lm_reference=ref, **kw)
        with pytest.raises(ValueError, match=msg):
            model.forward_backward(sb.input_ids, d["image_feat"], d["image_loc"], (1.0, 0.0, 0.0), lm_reference=ref,
                                   shared_context=sb.image_index, **kw)
