"""Knowledge distillation (DistillObjective + lm_reference) through the engine, the model surface and trainer.distill_step, on the
small configuration, T = 64, up to 8 sequences: alpha = 1 with a teacher against the step without the objective (bit for bit, both
schedules), the kernels on the model's own rows against the float64 restatement with the allowances of
tests/test_gpu_distill_edges.py, teachers of another depth and of another width (nothing of them changes, their logits are
released), the wiring (a frozen copy of the student is at KD ~ 0, a perturbed copy is not), ten steps of the loop body, the shared
schedule against the replicated one, and the launch order."""
import json
import math

import numpy as np
import pytest
import torch

from tests import distill_ref as DR
from tests.test_gpu_policy_kl_edges import U, grad_ratio
from tests.test_gpu_distill_edges import gate
from tests.test_gpu_policy_kl_model import assert_untouched, perturbed, run, snapshot
from tests.test_gpu_policy_model import CFG, fresh, step
from tests.test_gpu_shared_training import LOSS_TOL, sampled

pytestmark = pytest.mark.gpu
T, R = 64, 37


def teacher_of(seed=12, **over):
    """a frozen model of its own shape and weights: eval mode, no parameter asks for a gradient"""
    from oracle import vilbert_ref as RF
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    cfgd = json.load(open(CFG))
    cfgd.update(over)
    model = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd))
    sd = RF.init_state_dict(RF.make_config(cfgd), seed=seed)
    sd["cls.predictions.bias"] = torch.randn(sd["cls.predictions.bias"].shape, generator=torch.Generator().manual_seed(seed)) * 2.0
    model.load_state_dict(sd, strict=True)
    model.eval()
    model.requires_grad_(False)
    return model.cuda()


class Spy:
    """records what `_lm_loss_grad` reads and returns under a bound lm_objective.Distillation"""

    def __init__(self, model):
        self.engine, self.inner, self.calls = model.engine, model.engine._lm_loss_grad, []
        model.engine._lm_loss_grad = self

    def __call__(self, lm, g_lm):
        o = lm["objective"]
        rec = dict(ref=None if o.ref is None else o.ref.clone(), n=lm["n"], g=float(g_lm.reshape(-1)[0]),
                   count=lm["n"] if lm.get("n_dev") is None else int(lm["n_dev"][0]),
                   inv=float(lm["inv_dev"][0]) if lm.get("inv_dev") is not None else 1.0 / lm["n"],
                   **{k: lm[k].clone() for k in ("logits", "labels", "weights", "rowloss", "lse", "lse_t", "ref_lse_t", "kd")})
        rec["dlog"] = self.inner(lm, g_lm).clone()
        rec["released"] = o.ref is None
        self.calls.append(rec)
        return rec["dlog"]

    def close(self):
        self.engine._lm_loss_grad = self.inner


@pytest.fixture(scope="module")
def world():
    """one student, a shallow teacher, the student's perturbed frozen copy, an ordinary training batch of 8 sequences with
    likelihood and unlikelihood weights, and 3 dialogs x 2 answers for the shared schedule"""
    from unimm_amd import synth
    model = fresh()
    b = synth.make_batch(n_seq=8, T=T, R=R, cfg=model.config, seed=3, device="cuda")
    d, sb = sampled(2)
    return dict(model=model, shallow=teacher_of(num_hidden_layers=2, t_biattention_id=[0, 1]), far=perturbed(model), b=b, d=d, sb=sb)


def distill_kw(teacher, **obj):
    from unimm_amd.policy import DistillObjective
    return dict(lm_objective=DistillObjective(**obj), lm_reference=teacher)


def buckets_equal(model, new, old, tag):
    """every bucket of the gradient arena on which the three `old` runs agree among themselves is bit-equal in `new`; one that does
    not repeat (fp32 atomics on the word-embedding rows) is held to 2x their spread -> the number of such buckets"""
    noisy = 0
    for name, lo, hi in model.engine.arena.used_ranges():
        o = [r[1][lo:hi] for r in old]
        spread = max(float((o[i] - o[j]).abs().max()) for i, j in ((0, 1), (0, 2), (1, 2)))
        if spread == 0.0:
            assert torch.equal(new[1][lo:hi].view(torch.int32), o[0].view(torch.int32)), (tag, name)
        else:
            noisy += 1
            assert float((new[1][lo:hi] - o[0]).abs().max()) <= 2 * spread, (tag, name)
    return noisy


def test_alpha_one_with_a_teacher_is_todays_step(world):
    """DistillObjective(alpha=1) reads nothing of the teacher: same dropout seed and step as the step without the objective, the
    losses and the gradient arena bit for bit -- the replicated schedule on the ordinary batch with its likelihood and
    unlikelihood weights and all three loss terms, the shared schedule on the sampled answers.  No teacher forward runs."""
    model, teacher, b, d, sb = world["model"], world["shallow"], world["b"], world["d"], world["sb"]
    snap = snapshot(teacher)
    ran = []
    inner = teacher.engine.forward
    teacher.engine.forward = lambda *a, **k: ran.append(1) or inner(*a, **k)
    kw = distill_kw(teacher, temperature=3.0, alpha=1.0)
    try:
        assert int((b["lm_weight"][b["masked_lm_labels"] != -1] == -1).sum()) > 0 and int((b["lm_weight"] > 0).sum()) > 0
        old = [step(model, b, 7, lm_weight=b["lm_weight"]) for _ in range(3)]
        new = step(model, b, 7, lm_weight=b["lm_weight"], **kw)
        assert torch.equal(new[0].view(torch.int32), old[0][0].view(torch.int32)) and bool(torch.isfinite(new[0]).all())
        noisy = buckets_equal(model, new, old, "replicated")
        total = len(model.engine.arena.used_ranges())
        print(f"\nreplicated: {total - noisy} buckets bit-equal, {noisy} not reproducible in the step without the objective itself")
        assert noisy < total and float(new[1].abs().max()) > 0
        assert float(model.engine.last_lm_distill) == 0.0
        old = [run(model, d, sb, shared=True) for _ in range(3)]
        new = run(model, d, sb, shared=True, **kw)
        assert torch.equal(new[0].view(torch.int32), old[0][0].view(torch.int32)) and bool(torch.isfinite(new[0]).all())
        assert buckets_equal(model, new, old, "shared") == 0 and float(new[1].abs().max()) > 0
    finally:
        del teacher.engine.forward             # (the instance attribute: the class's method is back)
    assert not ran, "alpha = 1: no teacher forward"
    assert_untouched(teacher, snap)


def rows_against_reference(model, rec, tau, alpha, lm_loss, tag):
    """one recorded head: every output and the bf16 gradient against tests/distill_ref.py with the edge file's allowances"""
    V, n = model.config.vocab_size, rec["count"]
    z, zr = rec["logits"][:n, :V].cpu().numpy(), rec["ref"][:n, :V].cpu().numpy()
    y, w = rec["labels"][:n].cpu().numpy(), rec["weights"][:n].cpu().numpy()
    assert np.isfinite(z).all() and np.isfinite(zr).all()
    gs = float(np.float32(rec["g"]) * np.float32(rec["inv"]))
    assert abs(rec["inv"] - 1.0 / n) <= 1e-6 / n
    fw = DR.forward(z, zr, y, w, tau, alpha)
    grad_r = DR.backward(fw, y, w, gs)[0]
    al = DR.allowances(fw, z, zr, y, w, gs)
    f64 = lambda k: rec[k][:n].double().cpu().numpy()
    gate(f"({tag}) lse_t (abs / A_t)", np.abs(f64("lse_t") - fw["lse_t"]) / al["At"], 1.0)
    gate(f"({tag}) ref_lse_t (abs / A_t)", np.abs(f64("ref_lse_t") - fw["ref_lse_t"]) / al["Art"], 1.0)
    gate(f"({tag}) kd (abs / E_KD)", np.abs(f64("kd") - fw["kd"]) / al["EKD"], 1.0)
    gate(f"({tag}) rowloss (abs)", np.abs(f64("rowloss") - fw["rowloss"]), al["loss"])
    gd = rec["dlog"][:n].float().double().cpu().numpy()
    gate(f"({tag}) grad (err / allowance)", grad_ratio(gd[:, :V], grad_r, al["abs_err"]), 1.0)
    assert (gd[:, V:] == 0).all()
    assert abs(float(lm_loss) - fw["rowloss"].mean()) <= al["loss"].mean() + n * U * np.abs(fw["rowloss"]).max()
    return fw, al


def test_kernels_on_the_models_own_rows(world):
    """The student's and the teacher's logits rows of one train-mode step on the ordinary batch, as `_lm_loss_grad` reads them;
    lm_loss is the mean of the restatement's rowloss and engine.last_lm_distill the mean kd of the rows that took part."""
    model, teacher, b = world["model"], world["far"], world["b"]
    snap = snapshot(teacher)
    tau, alpha = 2.0, 0.5
    spy = Spy(model)
    try:
        losses, grads = step(model, b, 11, lm_weight=b["lm_weight"], **distill_kw(teacher, temperature=tau, alpha=alpha))
    finally:
        spy.close()
    rec = spy.calls[-1]
    assert rec["count"] == int((b["lm_weight"] != 0).sum())         # (given weights pick the decoded rows)
    assert rec["ref"].shape == rec["logits"].shape and rec["released"]
    assert rec["ref"].data_ptr() != rec["logits"].data_ptr() and not torch.equal(rec["ref"], rec["logits"])
    fw, al = rows_against_reference(model, rec, tau, alpha, losses[1], "model rows")
    w = rec["weights"][:rec["count"]].cpu().numpy()
    assert (w == -1).sum() >= 1 and (w > 0).sum() >= 1
    part = fw["part"]
    assert fw["kd"][part].min() > 1e-4, "the perturbed teacher is away from the student on every row"
    mean = float(model.engine.last_lm_distill)
    print(f"\nmean KD of {part.sum()} rows: engine {mean:.6f}, restatement {fw['kd'][part].mean():.6f}; lm_loss {float(losses[1]):.6f}")
    assert abs(mean - fw["kd"][part].mean()) <= al["EKD"][part].mean() + 2 * part.sum() * U * fw["kd"].max()
    assert model.engine.last_lm_distill.shape == (1,) and model.engine.last_lm_distill.dtype == torch.float32
    assert float(grads.abs().max()) > 0
    assert_untouched(teacher, snap)


@pytest.mark.parametrize("shape", ["shallow", "wide"])
def test_a_teacher_of_another_shape(world, shape):
    """A 2-layer teacher, and one of another hidden size, head count and intermediate size without frozen layers in common, both
    with other weights, against the 4-layer student: the step runs on both schedules, last_lm_distill is finite and above 1e-3,
    nothing of the teacher changed (parameters bitwise, no .grad, mode, its engine's dropout counters) and its logits are
    released after the backward.  The wide teacher's step also borrows a row capacity of 16 (`engine.lm_bucket`)."""
    model, b, d, sb = world["model"], world["b"], world["d"], world["sb"]
    if shape == "shallow":
        teacher, bucket = world["shallow"], 1
    else:
        teacher, bucket = teacher_of(seed=13, hidden_size=256, num_attention_heads=4, intermediate_size=384, fixed_t_layer=1), 16
    assert teacher.config.num_hidden_layers != model.config.num_hidden_layers or teacher.config.hidden_size != model.config.hidden_size
    snap = snapshot(teacher)
    model.engine.last_lm_kl = model.engine.last_lm_entropy = None
    was = model.engine.lm_bucket
    spy = Spy(model)
    try:
        model.engine.lm_bucket = bucket
        losses, grads = step(model, b, 5, lm_weight=b["lm_weight"], **distill_kw(teacher))
        kd_rep = float(model.engine.last_lm_distill)
        rec = spy.calls[-1]
        assert rec["n"] % bucket == 0 and rec["count"] == int((b["lm_weight"] != 0).sum()) and rec["ref"].shape[0] == rec["n"]
        assert teacher.engine.lm_bucket == 1                            # borrowed for the teacher's forward, given back
        model.engine.lm_bucket = was
        lm_shared, g_shared = run(model, d, sb, shared=True, **distill_kw(teacher))
        kd_shared = float(model.engine.last_lm_distill)
    finally:
        model.engine.lm_bucket = was
        spy.close()
    print(f"\n{shape} teacher: losses {losses.tolist()}, mean KD {kd_rep:.4f}; shared schedule lm_loss {float(lm_shared):.4f}, mean KD {kd_shared:.4f}")
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(lm_shared).all())
    assert float(grads.abs().max()) > 0 and float(g_shared.abs().max()) > 0 and bool(torch.isfinite(grads).all())
    for kd in (kd_rep, kd_shared):
        assert math.isfinite(kd) and kd > 1e-3
    assert all(c["released"] and c["ref"] is not None for c in spy.calls)
    assert model.engine.last_lm_kl is None and model.engine.last_lm_entropy is None
    rows_against_reference(model, rec, 2.0, 0.5, losses[1], f"{shape} teacher")
    assert_untouched(teacher, snap)


def test_wiring_a_copy_is_at_zero_a_perturbed_copy_is_not(world):
    """A student without dropout (every probability 0, train mode) against its own frozen copy in eval mode: the mean KD is at most
    the mean E_KD of its rows; against a perturbed copy it is at least 100x further."""
    from oracle import vilbert_ref as RF
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    from unimm_amd.policy import frozen_reference
    cfgd = json.load(open(CFG))
    cfgd.update({k: 0.0 for k in cfgd if k.endswith("dropout_prob")})
    student = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd))
    student.load_state_dict(RF.init_state_dict(RF.make_config(cfgd), seed=11), strict=True)
    student = student.cuda()
    same, far = frozen_reference(student), perturbed(student)
    assert not same.training and student is not same
    b = world["b"]
    got = {}
    for name, teacher in (("same", same), ("far", far)):
        spy = Spy(student)
        try:
            losses, _ = step(student, b, 3, lm_weight=b["lm_weight"], **distill_kw(teacher, temperature=2.0, alpha=0.0))
        finally:
            spy.close()
        rec = spy.calls[-1]
        fw, al = rows_against_reference(student, rec, 2.0, 0.0, losses[1], f"{name} copy")
        got[name] = (float(student.engine.last_lm_distill), float(al["EKD"][fw["part"]].mean()))
    print(f"\nmean KD against an identical copy {got['same'][0]:.3e} (E_KD {got['same'][1]:.1e}), against the perturbed copy {got['far'][0]:.3e}")
    assert -got["same"][1] <= got["same"][0] <= got["same"][1]
    assert got["far"][0] > 1e-3 and got["far"][0] >= 100 * max(got["same"][0], got["same"][1])


def test_ten_distill_steps_lower_the_distance(world):
    """trainer.distill_step with alpha = 0 on one fixed batch under one fixed dropout draw: after ten optimizer steps the mean KD to
    the teacher is lower than at the first; NSP and region terms train along, the teacher is untouched."""
    from unimm_amd import VisualDialogEncoder, synth, trainer
    from unimm_amd.optim import FusedAdamW, WarmupLinearScheduleNonZero, default_language_weights, reference_param_groups
    from unimm_amd.policy import DistillObjective
    torch.manual_seed(5)
    enc = VisualDialogEncoder(CFG).to("cuda")
    groups = reference_param_groups(enc, lr=2e-3, image_lr=2e-3, language_weights=default_language_weights(enc))
    eng = enc.bert_pretrained.engine
    opt = FusedAdamW(groups, eng, lr=2e-3)
    sch = WarmupLinearScheduleNonZero(opt, warmup_steps=1, t_total=40, min_lr=1e-5)
    teacher = world["shallow"]
    snap = snapshot(teacher)
    lb, nsp_w = synth.make_loader_batch(n_img=2, rounds=1, samples=3, T=T, cfg=enc.bert_pretrained.config, seed=100)
    batch = trainer.expand_image_fields(lb)
    params = dict(lm_loss_coeff=1.0, nsp_loss_coeff=1.0, img_loss_coeff=1.0, nsp_weight=nsp_w, batch_multiply=1)
    eng.ensure(torch.device("cuda", 0))
    p0 = eng.arena.flat.clone()
    kds, out = [], None
    for it in range(1, 11):
        enc.bert_pretrained.set_dropout_seed(9, step=0)
        out = trainer.distill_step(enc, opt, sch, batch, params, it, teacher=teacher, objective=DistillObjective(2.0, 0.0))
        kds.append(float(eng.last_lm_distill))
    torch.cuda.synchronize()
    print(f"\nmean KD over ten distill steps: {' '.join(f'{k:.4f}' for k in kds)}; last step {out}")
    assert len(out) == 4 and all(math.isfinite(v) for v in out) and all(math.isfinite(k) for k in kds)
    assert kds[-1] < kds[0] and kds[0] > 1e-3
    assert 0 < out[1] <= 4.0 * kds[-1] * (1 + 1e-5)                 # alpha = 0: lm_loss = tau^2 sum KD / #labelled rows (weight 0 included)
    assert enc.training and not teacher.training and opt.step_count == 10
    assert not torch.equal(p0, eng.arena.flat) and bool(torch.isfinite(eng.arena.flat).all())
    assert_untouched(teacher, snap)


def test_shared_and_replicated_schedules_agree(world):
    """eval mode (the two schedules draw their dropout masks at different sites): lm_loss and last_lm_distill of the shared step
    equal the replicated step's within the gate of tests/test_gpu_policy_kl_model.py for the same comparison."""
    model, teacher, d, sb = world["model"], world["shallow"], world["d"], world["sb"]
    got = {}
    for shared in (False, True):
        lm, _ = run(model, d, sb, shared=shared, train=False, **distill_kw(teacher, temperature=2.0, alpha=0.3))
        got[shared] = (float(lm), float(model.engine.last_lm_distill))
    print(f"\nreplicated lm_loss {got[False][0]:.6f} KD {got[False][1]:.6f}; shared lm_loss {got[True][0]:.6f} KD {got[True][1]:.6f}")
    for i in (0, 1):
        assert math.isfinite(got[True][i]) and abs(got[True][i] - got[False][i]) <= LOSS_TOL * max(abs(got[False][i]), 1e-3)
    assert got[False][1] > 1e-3


LOSS_ROWS = {"unimm_lm_loss_fwd", "unimm_lm_loss_bwd", "unimm_x3_lm_loss_bwd", "unimm_pg_loss_fwd", "unimm_pg_loss_bwd",
             "unimm_pg_kl_loss_fwd", "unimm_pg_kl_loss_bwd", "unimm_seq_pref", "unimm_distill_loss_fwd", "unimm_distill_loss_bwd"}


@pytest.mark.parametrize("shared", [False, True])
def test_launch_order(world, monkeypatch, shared):
    """The teacher's forward first (its own head runs the likelihood rows on the teacher's logits before handing them over), then
    unimm_distill_loss_fwd, later unimm_distill_loss_bwd; no unimm_lm_loss_* on the student's rows."""
    from unimm_amd import lib as L
    model, teacher, d, sb = world["model"], world["shallow"], world["d"], world["sb"]
    model.engine.ensure(torch.device("cuda", 0))
    names, inner = [], L._call
    in_teacher = []
    t_inner = teacher.engine.forward

    def recording(name, *args):
        names.append((name, bool(in_teacher)))
        return inner(name, *args)

    def teacher_forward(*a, **k):
        in_teacher.append(1)
        try:
            return t_inner(*a, **k)
        finally:
            in_teacher.pop()

    monkeypatch.setattr(L, "_call", recording)
    if not shared:
        teacher.engine.forward = teacher_forward
    try:
        lm_loss, grads = run(model, d, sb, shared=shared, **distill_kw(teacher))
    finally:
        monkeypatch.undo()
        if not shared:
            del teacher.engine.forward
    rows = [n for n, _ in names if n in LOSS_ROWS]
    assert rows == ["unimm_lm_loss_fwd", "unimm_distill_loss_fwd", "unimm_distill_loss_bwd"], rows
    if not shared:                             # the one likelihood launch is the teacher's, and all of the teacher's forward comes
        first = [n for n, _ in names].index("unimm_distill_loss_fwd")             # before the student's rows
        own = [i for i, (_, t) in enumerate(names) if t]
        assert [t for n, t in names if n == "unimm_lm_loss_fwd"] == [True] and own[-1] < first
        # ... and before the student's own forward: nothing of the student's encoder runs in between
        assert own == list(range(own[0], own[-1] + 1))
    assert bool(torch.isfinite(lm_loss).all()) and float(grads.abs().max()) > 0
