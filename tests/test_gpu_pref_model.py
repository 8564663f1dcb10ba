"""Preference training through the model (`lm_preference` / `PreferenceObjective`, unimm_amd/policy.py) on the small
configuration, T = 64: 2-3 dialogs x 4 candidates of 1-6 tokens, one of them absent.

1. the eval-mode loss against the fp64 formula applied to `sequence_log_likelihood` scores of the policy and the reference, on
   both schedules, with and without a reference, both length_normalize values.  Bound: 2 beta max_j (eS_j + eR_j) with e =
   (L_j + 2) 2^-24 sum_t |rownll_t| -- the loss is 1-Lipschitz in each z_j when W = 1 and e is the fp32 summation bound of a
   score (rownll >= 0, so sum_t |rownll_t| = |score|).
2. the backward's wiring.  Shared schedule, one dropout seed: a step with lm_preference leaves every gradient bit-equal to a
   step with lm_advantage = the adv rows the first step reported (LOGP mode), the common factor #rows / #alive = 16 / 2 = 8
   applied through the loss weight (a power of two: exact).  Replicated schedule: the word-embedding rows collect fp32 atomic
   adds there, so the comparison is held, bucket by bucket, to twice the spread three runs of the advantage step show among
   themselves (bit-equal where they agree bit for bit), the gate of tests/test_gpu_policy_model.py for the same situation.
   Measured on an MI355X: see WIRING_SPREAD below.
3. the shared against the replicated schedule, at the gates tests/test_gpu_shared_training.py holds the policy step to.
4. the reference is untouched by a step.  5. a reference equal to the policy: D = 0 exactly, P uniform, the entropy form.
6. one optimizer step lowers the eval-mode loss and raises the chosen candidates' P.  7. trainer.preference_step.
Also: a context that does not match its group's gives a NaN loss and adds nothing to the gradients, as for the other objectives."""
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_generate import make_dialogs
from tests.test_gpu_policy_model import CFG, T_TINY, fresh, policy_inputs
from tests.test_gpu_shared_training import LOSS_TOL, no_dropout

pytestmark = pytest.mark.gpu
# what three runs of the parent's advantage step showed among themselves on the wiring batch (replicated schedule), largest
# absolute difference per bucket; the test measures it again on every run and gates at twice what it measures
WIRING_SPREAD = "text_embeddings 2.8e-08 beside a largest gradient of 1.9e-01 (gate 5.6e-08); the other 10 buckets 0 (bit-equal)"
MAIN = [[1, 3, 0, 4], [2, 6, 5, 3], [4, 2, 6, 1]]
WIRING = [[1, 3, 0, 4], [2, 6, 0, 0]]                      # 16 rows, 2 groups: #rows / #alive = 8


def candidates(lengths, seed=3):
    """dialogs (contexts of different lengths) x candidates of the given lengths -> (dialogs, contexts, SampledBatch)"""
    from unimm_amd.policy import candidate_training_batch
    lengths = torch.tensor(lengths)
    G, N = lengths.shape
    d, c, _ = make_dialogs(G, T_TINY, 1000, 37, 192, seed=21, cmin=8, cmax=40)
    tokens = torch.from_numpy(np.random.default_rng(seed).integers(110, 1000, size=(G, N, 6)))
    return d, c, candidate_training_batch(d["input_ids"], d["token_type_ids"], d["position_ids"], c, tokens, lengths, T_TINY)


def targets(sb, kind="soft", seed=4):
    from unimm_amd.policy import PreferenceTargets, pair_targets, relevance_targets
    G, N = sb.shape
    if kind == "soft":
        w = relevance_targets(torch.from_numpy(np.random.default_rng(seed).integers(0, 5, (G, N)) * 0.5))
    else:
        w = pair_targets([1] * G, N)
    return PreferenceTargets(sb.image_index, w.reshape(-1)[sb.kept])


def step(model, d, sb, shared, seed=9, c_lm=1.0, **more):
    """one forward_backward from zeroed gradients under a fixed dropout seed -> (LM loss, gradient arena)"""
    model.engine.ensure(torch.device("cuda", 0))
    model.set_dropout_seed(seed, 0)
    model.engine.arena.zero_grads()
    kw = policy_inputs(sb, d, d["image_feat"].shape[0], model.config.v_target_size)
    kw.update(more)
    if shared:
        kw["shared_context"] = sb.image_index
    res = model.forward_backward(sb.input_ids, d["image_feat"], d["image_loc"], (c_lm, 0.0, 0.0), **kw)
    torch.cuda.synchronize()
    return res[1].clone(), model.engine.arena.grad_flat.clone()


def scores(model, d, sb, shared):
    model.eval()
    dev = "cuda"
    s, _ = model.sequence_log_likelihood(sb.input_ids.to(dev), d["image_feat"].to(dev), d["image_loc"].to(dev),
                                         sb.masked_lm_labels.to(dev), token_type_ids=sb.token_type_ids.to(dev),
                                         position_ids=sb.position_ids.to(dev), attention_mask=sb.attention_mask,
                                         image_attention_mask=d["image_attention_mask"][sb.image_index].to(dev),
                                         image_index=sb.image_index.to(dev), **(dict(shared_context=sb.image_index) if shared else {}))
    return s.double().cpu().numpy()


def host_loss(S, R, Ln, tg, beta, lnorm):
    """the fp64 formula on per-sequence scores -> (loss, P [B])"""
    z = float(np.float32(beta)) * (S - R) / (Ln if lnorm else 1.0)
    total, alive, P = 0.0, 0, np.zeros_like(z)
    for g in np.unique(tg.group):
        mem = np.flatnonzero(tg.group == g)
        w = tg.weight[mem].astype(np.float64)
        logP = z[mem] - (z[mem].max() + math.log(np.exp(z[mem] - z[mem].max()).sum()))
        P[mem] = np.exp(logP)
        if w.sum() > 0:
            total, alive = total - float((w * logP).sum()), alive + 1
    return total / alive, P


@pytest.fixture(scope="module")
def models():
    from unimm_amd.policy import frozen_reference
    model = fresh()
    ref = frozen_reference(model)
    with torch.no_grad():                                  # a reference that differs from the policy
        g = torch.Generator().manual_seed(1)
        for p in ref.parameters():
            p.add_((0.02 * torch.randn(p.shape, generator=g)).to(p.device) * p.abs().mean())
    ref.engine.invalidate_weights()
    return model, ref


@pytest.mark.parametrize("shared", [False, True])
def test_loss_equals_the_formula_on_sequence_scores(models, shared):
    from unimm_amd.policy import PreferenceObjective
    model, ref = models
    d, c, sb = candidates(MAIN)
    tg = targets(sb)
    Ln = sb.copy_rows.sum(1).double().numpy()
    S, R = scores(model, d, sb, shared), scores(ref, d, sb, shared)
    assert sb.input_ids.shape[0] == 11 and np.abs(S - R).max() > 1e-3
    model.eval()
    kw = policy_inputs(sb, d, d["image_feat"].shape[0], model.config.v_target_size)
    for use_ref in (False, True):
        for lnorm in (False, True):
            obj = PreferenceObjective(beta=0.5, length_normalize=lnorm)
            more = dict(lm_preference=tg, lm_objective=obj, **(dict(lm_reference=ref) if use_ref else {}))
            model.engine.last_lm_preference = None
            with torch.no_grad():
                got = model(sb.input_ids, d["image_feat"], d["image_loc"], **kw, **more,
                            **(dict(shared_context=sb.image_index) if shared else {}))[0]
            rep = model.engine.last_lm_preference
            Rj = R if use_ref else np.zeros_like(R)
            want, P = host_loss(S, Rj, Ln, tg, 0.5, lnorm)
            bound = 2 * 0.5 * float(((Ln + 2) * 2.0 ** -24 * (np.abs(S) + np.abs(Rj))).max())
            err = abs(float(got) - want)
            print(f"\nshared={shared} reference={use_ref} length_normalize={lnorm}: loss {float(got):.6f}, formula {want:.6f}, "
                  f"|difference| {err:.3e}, bound {bound:.3e}")
            assert math.isfinite(float(got)) and err <= bound
            assert np.abs(rep["seq_prob"].double().cpu().numpy() - P).max() <= 2 * bound + 2.0 ** -23
            assert set(rep) >= {"seq_score", "seq_prob", "group_loss", "adv"}


def test_backward_is_the_advantage_step_with_the_reported_rows(models):
    from unimm_amd.policy import PolicyObjective, PreferenceObjective
    model, ref = models
    d, c, sb = candidates(WIRING)
    tg = targets(sb)
    assert int(sb.copy_rows.sum()) == 16
    model.train()
    more = dict(lm_preference=tg, lm_objective=PreferenceObjective(beta=0.5), lm_reference=ref)

    def advantage_of(rep):
        """the reported adv rows as the [K, T] map lm_advantage takes: every copy row of sequence k holds c_k"""
        adv, seq = rep["adv"].cpu(), rep["row_seq"].cpu().long()
        out = torch.zeros(sb.copy_rows.shape, dtype=torch.float32)
        for k in range(sb.input_ids.shape[0]):
            mine = adv[seq == k]
            assert mine.numel() == int(sb.copy_rows[k].sum()) and bool((mine == mine[0]).all())
            out[k][sb.copy_rows[k]] = mine[0]
        assert bool((out != 0).any())
        return out

    # ---- shared schedule: bit for bit -------------------------------------------------------------------------------
    model.engine.last_lm_preference = None
    _, g_pref = step(model, d, sb, True, seed=77, **more)
    a = advantage_of(model.engine.last_lm_preference)
    _, g_adv = step(model, d, sb, True, seed=77, c_lm=8.0, lm_advantage=a, lm_objective=PolicyObjective(mode="logp"))
    assert float(g_pref.abs().max()) > 0 and torch.isfinite(g_pref).all()
    differ = [name for name, lo, hi in model.engine.arena.used_ranges()
              if not torch.equal(g_pref[lo:hi].view(torch.int32), g_adv[lo:hi].view(torch.int32))]
    assert not differ, differ
    # ---- replicated schedule: within twice the advantage step's own spread ------------------------------------------
    _, g_pref = step(model, d, sb, False, seed=77, **more)
    a = advantage_of(model.engine.last_lm_preference)
    old = [step(model, d, sb, False, seed=77, c_lm=8.0, lm_advantage=a, lm_objective=PolicyObjective(mode="logp"))[1] for _ in range(3)]
    noisy = []
    for name, lo, hi in model.engine.arena.used_ranges():
        o = [r[lo:hi] for r in old]
        spread = max(float((o[i] - o[j]).abs().max()) for i, j in ((0, 1), (0, 2), (1, 2)))
        if spread == 0.0:
            assert torch.equal(g_pref[lo:hi].view(torch.int32), o[0].view(torch.int32)), name
        else:
            diff = float((g_pref[lo:hi] - o[0]).abs().max())
            noisy.append(f"{name}: |preference - advantage| max {diff:.3e}, spread of three advantage runs {spread:.3e}, "
                         f"largest gradient {float(o[0].abs().max()):.3e}")
            assert diff <= 2 * spread, noisy[-1]
    print(f"\nreplicated: {len(model.engine.arena.used_ranges()) - len(noisy)} buckets bit-equal; not reproducible in the "
          f"advantage step itself: {noisy}")
    assert len(noisy) < len(model.engine.arena.used_ranges())


def test_shared_against_replicated_schedule():
    from unimm_amd.policy import PreferenceObjective, frozen_reference
    model = no_dropout(fresh())
    ref = frozen_reference(model)
    with torch.no_grad():
        for p in ref.parameters():
            p.mul_(1.01)
    d, c, sb = candidates(MAIN)
    model.train()
    _, like_r = step(model, d, sb, False)
    _, like_s = step(model, d, sb, True)
    yard = float((like_s - like_r).norm() / like_r.norm())
    more = dict(lm_preference=targets(sb), lm_objective=PreferenceObjective(beta=0.5), lm_reference=ref)
    lm_r, g_r = step(model, d, sb, False, **more)
    lm_s, g_s = step(model, d, sb, True, **more)
    got = float((g_s - g_r).norm() / g_r.norm())
    print(f"\nloss replicated {float(lm_r):.6f} shared {float(lm_s):.6f}; |shared - replicated| / |replicated| {got:.3e}, "
          f"likelihood run {yard:.3e}")
    assert torch.isfinite(g_s).all() and float(g_r.norm()) > 0
    assert abs(float(lm_s) - float(lm_r)) <= LOSS_TOL * max(abs(float(lm_r)), 1e-3)
    assert got <= 2 * yard


def test_mismatched_context_poisons_the_loss_and_adds_nothing(models):
    """the shared schedule's guard keeps its meaning: a context that is not its group's gives a NaN loss and adds nothing"""
    from types import SimpleNamespace
    from unimm_amd.policy import PreferenceObjective
    model, ref = models
    d, c, sb = candidates(MAIN)
    more = dict(lm_preference=targets(sb), lm_objective=PreferenceObjective(beta=0.5), lm_reference=ref)
    model.train()
    _, held = step(model, d, sb, True, **more)
    assert float(held.abs().max()) > 0
    bad = SimpleNamespace(**vars(sb))
    bad.input_ids = sb.input_ids.clone()
    bad.input_ids[5, 3] = 999 if int(sb.input_ids[5, 3]) != 999 else 998          # one context token of one member
    model.set_dropout_seed(9, 0)
    kw = policy_inputs(bad, d, d["image_feat"].shape[0], model.config.v_target_size)
    res = model.forward_backward(bad.input_ids, d["image_feat"], d["image_loc"], (1.0, 0.0, 0.0), shared_context=sb.image_index,
                                 **kw, **more)
    torch.cuda.synchronize()
    assert math.isnan(float(res[1])) and math.isnan(float(res[0]))
    assert torch.equal(model.engine.arena.grad_flat.view(torch.int32), held.view(torch.int32))


@pytest.mark.parametrize("shared", [False, True])
def test_the_reference_is_untouched(models, shared):
    from unimm_amd.policy import PreferenceObjective
    model, ref = models
    d, c, sb = candidates(MAIN)
    ref.engine.ensure(torch.device("cuda", 0))
    before = {k: v.clone() for k, v in ref.state_dict().items()}
    flat = ref.engine.arena.flat.clone()
    counters = (ref.engine.seed, ref.engine.step)
    model.train()
    lm, g = step(model, d, sb, shared, lm_preference=targets(sb), lm_objective=PreferenceObjective(), lm_reference=ref)
    assert math.isfinite(float(lm)) and float(g.abs().max()) > 0
    assert not ref.training and (ref.engine.seed, ref.engine.step) == counters
    assert all(p.grad is None and not p.requires_grad for p in ref.parameters())
    assert torch.equal(ref.engine.arena.flat.view(torch.int32), flat.view(torch.int32))
    for k, v in ref.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_a_reference_equal_to_the_policy():
    from unimm_amd.policy import PreferenceObjective, frozen_reference
    model = fresh().eval()
    ref = frozen_reference(model)
    d, c, sb = candidates(MAIN)
    tg = targets(sb)
    for lnorm in (False, True):
        lm, _ = step(model, d, sb, True, lm_preference=tg, lm_objective=PreferenceObjective(0.5, lnorm), lm_reference=ref)
        rep = model.engine.last_lm_preference
        assert bool((rep["seq_score"] == 0).all())                                    # D = 0 exactly
        M = np.bincount(tg.group)[tg.group].astype(np.float64)
        P = rep["seq_prob"].double().cpu().numpy()
        assert np.abs(P - 1.0 / M).max() <= 2.0 ** -24 * (1.0 / M).max()
        want = np.mean([-(tg.weight[tg.group == g].astype(np.float64) * math.log(1.0 / (tg.group == g).sum())).sum()
                        for g in np.unique(tg.group)])
        assert abs(float(lm) - want) <= 4 * 2.0 ** -24 * want


def test_one_optimizer_step_lowers_the_loss():
    from unimm_amd import VisualDialogEncoder
    from unimm_amd.optim import FusedAdamW, default_language_weights, reference_param_groups
    from unimm_amd.policy import PreferenceObjective
    torch.manual_seed(5)
    enc = VisualDialogEncoder(CFG).to("cuda")
    model = no_dropout(enc.bert_pretrained)
    groups = reference_param_groups(enc, lr=2e-5, image_lr=2e-5, language_weights=default_language_weights(enc))
    opt = FusedAdamW(groups, model.engine, lr=2e-5)
    d, c, sb = candidates([[3, 4, 0, 0], [2, 5, 0, 0]])
    tg = targets(sb, kind="pair")                                                    # candidate 1 of each dialog is the chosen one
    chosen = torch.from_numpy(tg.weight > 0)
    obj = PreferenceObjective(beta=0.5)

    def evaluate():
        model.eval()
        lm, _ = step(model, d, sb, True, lm_preference=tg, lm_objective=obj)
        return float(lm), model.engine.last_lm_preference["seq_prob"].cpu()[chosen].clone()

    before, p_before = evaluate()
    model.train()
    step(model, d, sb, True, lm_preference=tg, lm_objective=obj)
    opt.step()
    opt.zero_grad()
    after, p_after = evaluate()
    print(f"\neval-mode loss {before:.6f} -> {after:.6f}; P of the chosen candidates {p_before.tolist()} -> {p_after.tolist()}")
    assert math.isfinite(after) and after < before and bool((p_after > p_before).all())


@pytest.mark.parametrize("shared", [False, True])
def test_preference_step(shared):
    from unimm_amd import VisualDialogEncoder, trainer
    from unimm_amd.optim import FusedAdamW, WarmupLinearScheduleNonZero, default_language_weights, reference_param_groups
    from unimm_amd.policy import PreferenceObjective, frozen_reference, relevance_targets
    torch.manual_seed(5)
    enc = VisualDialogEncoder(CFG).to("cuda")
    groups = reference_param_groups(enc, lr=1e-3, image_lr=4e-3, language_weights=default_language_weights(enc))
    opt = FusedAdamW(groups, enc.bert_pretrained.engine, lr=1e-3)
    sch = WarmupLinearScheduleNonZero(opt, warmup_steps=2, t_total=20, min_lr=1e-5)
    ref = frozen_reference(enc)
    eng = enc.bert_pretrained.engine
    assert eng.last_lm_preference is None
    lengths = torch.tensor(MAIN)
    G, N = lengths.shape
    d, c, _ = make_dialogs(G, T_TINY, 1000, 37, 192, seed=21, cmin=8, cmax=40)
    rng = np.random.default_rng(6)
    w = relevance_targets(torch.from_numpy(rng.integers(0, 5, (G, N)) * 0.5))
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"],
                 answer_tokens=torch.from_numpy(rng.integers(110, 1000, size=(G, N, 6))), answer_lengths=lengths, targets=w)
    eng.ensure(torch.device("cuda", 0))
    p0 = eng.arena.flat.clone()
    for it in (1, 2):
        out = trainer.preference_step(enc, opt, sch, batch, dict(batch_multiply=2), it, objective=PreferenceObjective(0.5, True),
                                      reference=ref, shared_context=shared)
        torch.cuda.synchronize()
        assert len(out) == 3 and all(math.isfinite(v) for v in out), out
        assert torch.equal(p0, eng.arena.flat) == (it == 1)                           # the update comes with the second micro-batch
        # the diagnostics, recomputed from what the step left behind
        D = eng.last_lm_preference["seq_score"].double().cpu().numpy()
        keep = (lengths.reshape(-1) > 0).numpy()
        Dg = np.full(G * N, np.nan)
        Dg[keep] = D
        Dg, wg = Dg.reshape(G, N), w.double().numpy()
        hit, margin = [], []
        for g in range(G):
            top = int(np.argmax(np.where(keep.reshape(G, N)[g], wg[g], -1.0)))
            hit.append(float(int(np.nanargmax(Dg[g])) == top))
            others = [j for j in range(N) if j != top and keep.reshape(G, N)[g, j]]
            wo = wg[g, others] if wg[g, others].sum() > 0 else np.ones(len(others))
            margin.append(Dg[g, top] - float((wo * Dg[g, others]).sum() / wo.sum()))
        assert out[1] == pytest.approx(np.mean(hit), abs=1e-12) and out[2] == pytest.approx(np.mean(margin), rel=1e-9, abs=1e-12)
    assert torch.isfinite(eng.arena.flat).all()
    with pytest.raises(ValueError, match="at most 30 tokens"):
        trainer.preference_step(enc, opt, sch, dict(batch, answer_lengths=lengths + 31), dict(batch_multiply=1), 3, shared_context=True)
