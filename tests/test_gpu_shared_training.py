"""The shared-context training step (`forward_backward(shared_context=...)`, unimm_amd/scoring.py `train_shared`) on the small
configuration, T = 64: N sampled answers of a dialog as N sequences of one group, context and image computed once, forward
and backward.

(a) against the replicated step (the same sequences, each with its own copy of the context) and the CPU oracle's autograd
    (oracle/vilbert_ref.py, likelihood on the copy rows): 3 dialogs with contexts of different lengths, N in {1, 4} answers of
    1 .. 6 tokens, no dropout.  e = relative L2 error of all parameter gradients against the oracle; required
    e_shared <= 1.5 e_replicated.  The factor is a margin between two legitimate summation orders: the replicated step rounds N
    per-copy context gradients to bf16 before the weight-gradient GEMMs add them, the shared step adds first; a dropped or
    doubled contribution is an error of order 1 / N.  The loss agrees with the replicated step's to 2e-3 (the tolerance of
    tests/test_gpu_fullsize.py for shared versus per-candidate scores).  The policy objectives have no oracle: their
    shared-versus-replicated gradient difference must stay within 2x of the likelihood run's (the objective changes only the
    row kernels' inputs).
(b) dropout on: the same seed twice is bit-identical, another seed differs, everything finite.
    (the step's embedding gradient is added in a fixed order, `Engine._embed_text_bwd_ordered`: the replicated step's fp32 atomics
    into the word-embedding rows are the one thing in it that does not repeat)
(c) a context that does not match its group's: NaN loss, the gradient arena bit-identical to what it held.
(d) every gradient bucket handed over exactly once, the same set as in the replicated step.
(e) trainer.self_critical_step(shared_context=True) with the baselines / objectives of tests/test_gpu_policy_model.py."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_gpu_generate import make_dialogs
from tests.test_gpu_policy_model import MAXLEN, T_TINY, _encoder, fresh, policy_inputs, tiny_dialogs

pytestmark = pytest.mark.gpu
LOSS_TOL = 2e-3


def sampled(N, seed=3, G=3):
    """G dialogs (contexts of different lengths) x N answers of 1 .. 6 random tokens -> (dialogs, SampledBatch)"""
    from unimm_amd.policy import sampled_training_batch
    d, c, _ = make_dialogs(G, T_TINY, 1000, 37, 192, seed=21, cmin=8, cmax=40)
    assert len(set(int(x) for x in c)) == G, c
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 7, size=(G, N))
    lengths[0, 0], lengths[-1, -1] = 1, 6
    tokens = rng.integers(110, 1000, size=(G, N, 6))
    ans = SimpleNamespace(tokens=torch.from_numpy(tokens), lengths=torch.from_numpy(lengths))
    return d, sampled_training_batch(d["input_ids"], d["token_type_ids"], d["position_ids"], c, ans, T_TINY)


def run(model, d, sb, shared, seed=9, zero=True, **more):
    """one step from zeroed gradients under a fixed dropout seed -> (LM loss, gradient arena)"""
    model.train()
    model.engine.ensure(torch.device("cuda", 0))
    model.set_dropout_seed(seed, 0)
    if zero:
        model.engine.arena.zero_grads()
    kw = policy_inputs(sb, d, d["image_feat"].shape[0], model.config.v_target_size)
    kw.update(more)
    if shared:
        kw["shared_context"] = sb.image_index
    res = model.forward_backward(sb.input_ids, d["image_feat"], d["image_loc"], (1.0, 0.0, 0.0), **kw)
    torch.cuda.synchronize()
    return res, model.engine.arena.grad_flat.clone()


def no_dropout(model):
    for k in ("hidden_dropout_prob", "attention_probs_dropout_prob", "v_hidden_dropout_prob", "v_attention_probs_dropout_prob"):
        setattr(model.config, k, 0.0)
        setattr(model.engine.cfg, k, 0.0)
    return model


def oracle_grads(model, d, sb):
    """autograd of the CPU oracle: mean cross-entropy on the copy rows -> {parameter name: gradient}"""
    from oracle import vilbert_ref as R
    import json
    from tests.test_gpu_policy_model import CFG
    ocfg = R.make_config(json.load(open(CFG)))
    for k in ("hidden_dropout_prob", "attention_probs_dropout_prob", "v_hidden_dropout_prob", "v_attention_probs_dropout_prob"):
        setattr(ocfg, k, 0.0)
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k != R.TIED[0]}
    leaves[R.TIED[0]] = leaves[R.TIED[1]]
    txt, co = sb.attention_mask.dense(T_TINY)
    K, Rr = sb.input_ids.shape[0], d["image_feat"].shape[1]
    ix = sb.image_index
    out = R.trunk(leaves, ocfg, sb.input_ids, d["image_feat"][ix], d["image_loc"][ix], sb.token_type_ids, sb.position_ids,
                  torch.from_numpy(np.asarray(txt)).float(), d["image_attention_mask"][ix].float(),
                  torch.from_numpy(np.asarray(co)).float()[:, None, :].expand(K, Rr, T_TINY))
    pred_t, _, _ = R.heads(leaves, ocfg, *out)
    R.mlm_ul_loss(pred_t, sb.masked_lm_labels, None).backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


def rel_errors(model, flat, want):
    """relative L2 error of all parameter gradients (the arena `flat`) against `want`, and per gradient bucket"""
    arena = model.engine.arena
    flat = flat.double().cpu()
    num = den = 0.0
    per = {g: [0.0, 0.0] for g, _, _ in arena.buckets}
    for name in arena.params:
        o, shape = arena.offsets[name]
        w = want[name].detach().double().reshape(-1)
        got = flat[o:o + w.numel()]
        n_, d_ = float(((got - w) ** 2).sum()), float((w ** 2).sum())
        num, den = num + n_, den + d_
        g = next(g for g, lo, hi in arena.buckets if lo <= o < hi)
        per[g][0] += n_
        per[g][1] += d_
    return math.sqrt(num / den), {k: math.sqrt(v[0] / v[1]) for k, v in per.items() if v[1] > 0}


@pytest.fixture(scope="module")
def likelihood_runs():
    """(a), likelihood objective, for N = 1 and N = 4: both steps' losses and gradient arenas, the oracle's gradients"""
    model = no_dropout(fresh())
    res = {}
    for N in (1, 4):
        d, sb = sampled(N)
        (_, lm_r, _, _, _), g_r = run(model, d, sb, False)
        (loss_s, lm_s, img_s, nsp_s, logits_s), g_s = run(model, d, sb, True)
        assert logits_s is None and float(img_s) == 0.0 and float(nsp_s) == 0.0 and float(loss_s) == float(lm_s)
        res[N] = dict(model=model, d=d, sb=sb, lm_r=float(lm_r), lm_s=float(lm_s), g_r=g_r, g_s=g_s, want=oracle_grads(model, d, sb))
    return res


@pytest.mark.parametrize("N", [1, 4])
def test_shared_step_against_replicated_step_and_oracle(likelihood_runs, N):
    r = likelihood_runs[N]
    e_rep, per_rep = rel_errors(r["model"], r["g_r"], r["want"])
    e_sh, per_sh = rel_errors(r["model"], r["g_s"], r["want"])
    print(f"\nN = {N}: loss replicated {r['lm_r']:.6f} shared {r['lm_s']:.6f}; gradient error against the oracle: "
          f"replicated {e_rep:.3e}, shared {e_sh:.3e}")
    for k in sorted(per_rep):
        print(f"    {k}: replicated {per_rep[k]:.3e} shared {per_sh[k]:.3e}")
    assert math.isfinite(r["lm_s"]) and abs(r["lm_s"] - r["lm_r"]) <= LOSS_TOL * abs(r["lm_r"])
    assert e_sh <= 1.5 * e_rep, (e_sh, e_rep)


@pytest.mark.parametrize("objective_kw", [dict(mode="logp"), dict(mode="ratio", clip_eps=0.2)])
def test_policy_objectives_shared_against_replicated(likelihood_runs, objective_kw):
    from unimm_amd.policy import PolicyObjective, spread
    r = likelihood_runs[4]
    model, d, sb = r["model"], r["d"], r["sb"]
    yard = float((r["g_s"] - r["g_r"]).norm() / r["g_r"].norm())
    G, N = sb.shape
    rng = torch.Generator().manual_seed(2)
    adv = torch.randn((G, N), generator=rng)
    assert bool((adv > 0).any()) and bool((adv < 0).any())
    more = dict(lm_advantage=spread(adv, sb), lm_objective=PolicyObjective(**objective_kw))
    if objective_kw["mode"] == "ratio":
        more["lm_behaviour_logp"] = spread(-6.5 + 0.5 * torch.randn((G, N, 6), generator=rng), sb)
    (_, lm_r, _, _, _), g_r = run(model, d, sb, False, **more)
    (_, lm_s, _, _, _), g_s = run(model, d, sb, True, **more)
    got = float((g_s - g_r).norm() / g_r.norm())
    print(f"\n{objective_kw}: loss replicated {float(lm_r):.6f} shared {float(lm_s):.6f}; |shared - replicated| / |replicated| "
          f"{got:.3e}, likelihood run {yard:.3e}")
    assert torch.isfinite(g_s).all() and float(g_r.norm()) > 0
    assert abs(float(lm_s) - float(lm_r)) <= LOSS_TOL * max(abs(float(lm_r)), 1e-3)
    assert got <= 2 * yard


def test_dropout_seed_fixes_the_step():
    model = fresh()
    d, sb = sampled(4)
    (_, l1, _, _, _), g1 = run(model, d, sb, True, seed=31)
    (_, l2, _, _, _), g2 = run(model, d, sb, True, seed=31)
    (_, l3, _, _, _), g3 = run(model, d, sb, True, seed=32)
    assert torch.isfinite(g1).all() and torch.isfinite(g3).all() and math.isfinite(float(l1)) and math.isfinite(float(l3))
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    differ = [name for name, lo, hi in model.engine.arena.used_ranges() if not torch.equal(g1[lo:hi].view(torch.int32), g2[lo:hi].view(torch.int32))]
    print(f"\nbuckets that differ between two runs of one seed: {differ}")
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)), differ
    assert float(l1) != float(l3) and not torch.equal(g1, g3)


def test_mismatched_context_poisons_the_loss_and_adds_nothing():
    model = no_dropout(fresh())
    d, sb = sampled(4)
    _, held = run(model, d, sb, True)                            # the arena holds a step's gradients
    assert float(held.abs().max()) > 0
    bad = SimpleNamespace(**vars(sb))
    bad.input_ids = sb.input_ids.clone()
    bad.input_ids[5, 3] = 999 if int(sb.input_ids[5, 3]) != 999 else 998      # one context token of one member
    (loss, lm, _, _, _), after = run(model, d, bad, True, zero=False)
    assert math.isnan(float(lm)) and math.isnan(float(loss))
    assert torch.equal(after.view(torch.int32), held.view(torch.int32))


def test_every_bucket_handed_over_once():
    model = no_dropout(fresh())
    d, sb = sampled(4)
    seen = {}
    model.engine.ensure(torch.device("cuda", 0))
    for shared in (False, True):
        got = seen[shared] = []
        model.engine.grad_bucket_hook = lambda g, more, got=got: got.append(g)
        run(model, d, sb, shared)
    model.engine.grad_bucket_hook = None
    assert len(seen[True]) == len(set(seen[True])), seen[True]
    assert set(seen[True]) == set(seen[False]) and len(seen[False]) == len(set(seen[False]))


@pytest.mark.parametrize("baseline,objective_kw,sample_kw", [
    ("greedy", dict(), dict()),
    ("mean", dict(entropy_coef=0.01), dict()),
    ("mean", dict(mode="ratio", clip_eps=0.2, entropy_coef=0.01), dict(top_k=20, temperature=0.8)),
])
def test_self_critical_step_shared(baseline, objective_kw, sample_kw):
    from unimm_amd import trainer
    from unimm_amd.policy import PolicyObjective
    d, c, _ = tiny_dialogs(G=4, seed=8)
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"])
    reward = lambda tokens, lengths: -lengths.float()
    losses = {}
    for shared in (False, True):
        enc, opt, sch = _encoder()
        no_dropout(enc.bert_pretrained)
        eng = enc.bert_pretrained.engine
        eng.ensure(torch.device("cuda", 0))
        p0 = eng.arena.flat.clone()
        out = trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), 1, reward, samples=3, baseline=baseline,
                                         objective=PolicyObjective(**objective_kw), max_answer_len=MAXLEN, seed=4,
                                         shared_context=shared, **sample_kw)
        torch.cuda.synchronize()
        assert all(math.isfinite(v) for v in out), out
        assert not torch.equal(p0, eng.arena.flat) and torch.isfinite(eng.arena.flat).all()
        losses[shared] = out[0]
    print(f"\nself_critical_step({baseline}, {objective_kw}): loss replicated {losses[False]:.6f} shared {losses[True]:.6f}")
    assert abs(losses[True] - losses[False]) <= LOSS_TOL * max(abs(losses[False]), 1e-3)
