"""The shared-context pass with answers of up to 30 tokens (`SharedContext(groups, 64)`: two query tiles of private rows,
unimm_attn_spliced_wide_fwd / _bwd) on the small configuration, T = 64, with the helpers of tests/test_gpu_shared_training.py.

Three dialogs with contexts of 8 .. 20 tokens, N = 4 answers each with lengths from {1, 14, 15, 16, 21}: every group mixes
members of one query tile (at most 14 tokens) and of two.

(a) training, no dropout: the wide shared step against the replicated step and the CPU oracle's autograd.  Loss within LOSS_TOL;
    e_shared <= 1.5 e_replicated, the margin tests/test_gpu_shared_training.py argues for (two legitimate summation orders; a
    dropped contribution is an error of order 1 / N).
(b) training, dropout on: one seed twice is bit-identical, another seed differs, everything finite.
(c) a SharedContext(.., 64) step whose answers all have at most 14 tokens has the loss and gradient arena BITS of the bare-list
    step under one seed, dropout on: the permission does not change the launches.
(d) scoring on both engines: sequence_log_likelihood(shared_context=SharedContext(g, 64)) against the per-candidate call on
    candidates of 1 .. 21 tokens; bf16 within 2e-3 of the largest |score| (tests/test_gpu_fullsize.py), fp32x3 within
    1e-3 + 1e-3 |want| (tests/test_gpu_x3_scoring.py).
(e) trainer.self_critical_step(shared_context=True, max_answer_len=20, samples=3): finite, the parameters move, the loss within
    LOSS_TOL of the shared_context=False step; at least one trained answer has more than 14 tokens (else the test has shown
    nothing, and says so); max_answer_len = 31 raises.
(f) trainer.generative_evaluate(shared_context=True): one image, 2 rounds of 5 options, one option of 16 tokens; ranks equal the
    default call's wherever the per-candidate scores of two candidates differ by more than the score tolerance."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_gpu_generate import make_dialogs
from tests.test_gpu_policy_model import T_TINY, _encoder, fresh
from tests.test_gpu_shared_training import LOSS_TOL, no_dropout, oracle_grads, rel_errors, run, sampled

pytestmark = pytest.mark.gpu
LENGTHS = np.array([[1, 15, 14, 21], [16, 1, 21, 14], [14, 15, 16, 21]])


def short_dialogs(G, cmax=20):
    """G dialog contexts of 8 .. cmax tokens, all of different lengths (the first seed that gives them)"""
    for seed in range(200):
        d, c, _ = make_dialogs(G, T_TINY, 1000, 37, 192, seed=seed, cmin=8, cmax=cmax)
        if len(set(int(x) for x in c)) == G and 8 <= int(c.min()) and int(c.max()) <= cmax:
            return d, c
    raise AssertionError("no seed gives contexts of 8 .. 20 tokens")


def wide_sampled():
    """-> (dialogs, SampledBatch) of 3 dialogs x 4 answers with LENGTHS tokens"""
    from unimm_amd.policy import sampled_training_batch
    d, c = short_dialogs(3)
    tokens = np.random.default_rng(3).integers(110, 1000, size=(3, 4, 21))
    ans = SimpleNamespace(tokens=torch.from_numpy(tokens), lengths=torch.from_numpy(LENGTHS))
    sb = sampled_training_batch(d["input_ids"], d["token_type_ids"], d["position_ids"], c, ans, T_TINY)
    assert sb.input_ids.shape[0] == 12
    return d, sb


def ctx64(sb):
    from unimm_amd import SharedContext
    return SharedContext(sb.image_index, 64)


def test_wide_shared_step_against_replicated_step_and_oracle():
    model = no_dropout(fresh())
    d, sb = wide_sampled()
    with pytest.raises(ValueError, match="32-row query tile"):       # the bare list still refuses this batch
        run(model, d, sb, True)
    (_, lm_r, _, _, _), g_r = run(model, d, sb, False)
    (loss_s, lm_s, img_s, nsp_s, logits_s), g_s = run(model, d, sb, False, shared_context=ctx64(sb))
    assert logits_s is None and float(img_s) == 0.0 and float(nsp_s) == 0.0 and float(loss_s) == float(lm_s)
    want = oracle_grads(model, d, sb)
    e_rep, per_rep = rel_errors(model, g_r, want)
    e_sh, per_sh = rel_errors(model, g_s, want)
    print(f"\nwide: loss replicated {float(lm_r):.6f} shared {float(lm_s):.6f}; gradient error against the oracle: "
          f"replicated {e_rep:.3e}, shared {e_sh:.3e}")
    for k in sorted(per_rep):
        print(f"    {k}: replicated {per_rep[k]:.3e} shared {per_sh[k]:.3e}")
    assert math.isfinite(float(lm_s)) and abs(float(lm_s) - float(lm_r)) <= LOSS_TOL * abs(float(lm_r))
    assert e_sh <= 1.5 * e_rep, (e_sh, e_rep)


def test_wide_dropout_seed_fixes_the_step():
    model = fresh()
    d, sb = wide_sampled()
    (_, l1, _, _, _), g1 = run(model, d, sb, False, seed=31, shared_context=ctx64(sb))
    (_, l2, _, _, _), g2 = run(model, d, sb, False, seed=31, shared_context=ctx64(sb))
    (_, l3, _, _, _), g3 = run(model, d, sb, False, seed=32, shared_context=ctx64(sb))
    assert torch.isfinite(g1).all() and torch.isfinite(g3).all() and math.isfinite(float(l1)) and math.isfinite(float(l3))
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    differ = [name for name, lo, hi in model.engine.arena.used_ranges() if not torch.equal(g1[lo:hi].view(torch.int32), g2[lo:hi].view(torch.int32))]
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)), differ
    assert float(l1) != float(l3) and not torch.equal(g1, g3)


def test_permission_alone_changes_no_bit():
    model = fresh()
    d, sb = sampled(4)                                               # answers of 1 .. 6 tokens
    (_, l_bare, _, _, _), g_bare = run(model, d, sb, True, seed=31)
    (_, l_wide, _, _, _), g_wide = run(model, d, sb, False, seed=31, shared_context=ctx64(sb))
    assert math.isfinite(float(l_bare)) and float(g_bare.abs().max()) > 0
    assert torch.equal(l_bare.view(torch.int32), l_wide.view(torch.int32))
    assert torch.equal(g_bare.view(torch.int32), g_wide.view(torch.int32))


@pytest.mark.parametrize("compute", ["bf16", "fp32x3"])
def test_wide_scoring_against_per_candidate(compute):
    from unimm_amd import SharedContext, synth
    model = fresh(compute).eval()
    for seed in range(100):                                          # the first batch with candidates of 1 and of 21 tokens
        b = synth.make_scoring_batch(rounds=3, options=6, T=T_TINY, cfg=model.config, seed=seed, a_range=(1, 21), c_range=(8, 20), device="cuda")
        n = torch.as_tensor(b["mask_spec"].answer) - 1
        if int(n.max()) == 21 and int(n.min()) == 1:
            break
    spec = b.pop("mask_spec")
    assert int(n.max()) == 21 and int(n.min()) == 1 and int((n > 14).sum()) >= 3 and int((n <= 14).sum()) >= 3
    args = (b["input_ids"], b["image_feat"], b["image_loc"], b["masked_lm_labels"])
    kw = dict(token_type_ids=b["token_type_ids"], position_ids=b["token_position_ids"], attention_mask=b["attention_mask"],
              co_attention_mask=b["co_attention_mask"], image_attention_mask=b["image_attention_mask"])
    grp = b["context_group"]
    with pytest.raises(ValueError, match="32-row query tile"):
        model.sequence_log_likelihood(*args, shared_context=grp, **kw)
    base, _ = model.sequence_log_likelihood(*args, **kw)
    got, _ = model.sequence_log_likelihood(*args, shared_context=SharedContext(grp, 64), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and (got < 0).all()
    d = (got - base).abs()
    print(f"\n{compute}: tokens {n.tolist()}; shared vs per-candidate max |d| {float(d.max()):.3e} on scale {float(base.abs().max()):.3g}")
    if compute == "bf16":
        assert float(d.max()) <= 2e-3 * float(base.abs().max())
    else:
        assert bool((d <= 1e-3 + 1e-3 * base.abs()).all()), float(d.max())


def test_self_critical_step_shared_default_answer_length():
    from unimm_amd import trainer
    d, c = short_dialogs(4, cmax=22)                                 # 22 + 2 (20 + 1) = 64 = T
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"])
    losses, seen = {}, {}
    for shared in (False, True):
        lengths = seen[shared] = []

        def reward(tokens, lens, lengths=lengths):                   # a toy host reward that tells the samples apart
            lengths.append(lens.clone())
            return (tokens.float() % 13.0).mean(-1) - lens.float()
        enc, opt, sch = _encoder()
        no_dropout(enc.bert_pretrained)
        eng = enc.bert_pretrained.engine
        eng.ensure(torch.device("cuda", 0))
        p0 = eng.arena.flat.clone()
        out = trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), 1, reward, samples=3, max_answer_len=20, seed=4,
                                         shared_context=shared)
        torch.cuda.synchronize()
        assert all(math.isfinite(v) for v in out), out
        assert not torch.equal(p0, eng.arena.flat) and torch.isfinite(eng.arena.flat).all()
        losses[shared] = out[0]
    sampled_lengths = seen[True][0]                                  # the first reward call scores the samples
    assert sampled_lengths.shape == (4, 3)
    assert int(sampled_lengths.max()) > 14, ("no sampled answer has more than 14 tokens: this run shows nothing about the two-tile "
                                             f"launches (lengths {sampled_lengths.tolist()})")
    print(f"\nself_critical_step, max_answer_len 20: sampled lengths {sampled_lengths.tolist()}; loss replicated {losses[False]:.6f} "
          f"shared {losses[True]:.6f}")
    assert losses[False] != 0.0, "every advantage is zero: the two losses were not compared"
    assert abs(losses[True] - losses[False]) <= LOSS_TOL * max(abs(losses[False]), 1e-3)
    enc, opt, sch = _encoder()
    with pytest.raises(ValueError, match="at most 30 tokens"):
        trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), 1, reward, samples=3, max_answer_len=31, shared_context=True)


def test_generative_evaluate_shared_context():
    from unimm_amd import synth, trainer
    from unimm_amd.harness import scores_to_ranks
    enc, _, _ = _encoder()
    cfg = enc.bert_pretrained.config
    rounds, options = 2, 5
    for seed in range(200):                                          # the first batch whose longest option has exactly 16 tokens
        s = synth.make_scoring_batch(rounds=rounds, options=options, T=T_TINY, cfg=cfg, seed=seed, a_range=(1, 16), c_range=(8, 24))
        n = torch.as_tensor(s["mask_spec"].answer) - 1
        if int((n == 16).sum()) == 1:
            break
    assert int((n == 16).sum()) == 1 and int(n.max()) == 16
    s.pop("mask_spec")
    shp = lambda t: t.reshape((1, rounds, options) + tuple(t.shape[1:]))
    K = rounds * options
    b = dict(tokens=shp(s["input_ids"]), segments=shp(s["token_type_ids"]), positions=shp(s["token_position_ids"]),
             mask=shp(s["masked_lm_labels"]), weights=torch.ones((1, rounds, options, T_TINY)), sep_indices=torch.zeros((1, rounds, options, 1), dtype=torch.int64),
             hist_len=torch.zeros((1, rounds, options), dtype=torch.int64), txt_attention_mask=shp(s["attention_mask"]),
             co_attention_mask=shp(s["co_attention_mask"]), image_feat=s["image_feat"][:1], image_loc=s["image_loc"][:1],
             image_mask=s["image_attention_mask"][:1], gt_option_inds=torch.tensor([[2, 0]]),
             gt_relevance=torch.tensor([[0, 0.5, 1.0, 0, 0.2]]), round_id=torch.tensor([[1]]))
    params = dict(n_gpus=1, nsp_weight=None)
    r_def, r_sh = [], []
    m_def = trainer.generative_evaluate([b], params, 1, enc, chunk_size=K, ranks_out=r_def)
    m_sh = trainer.generative_evaluate([b], params, 1, enc, chunk_size=K, ranks_out=r_sh, shared_context=True)
    m_sh5 = trainer.generative_evaluate([b], params, 1, enc, chunk_size=options, shared_context=True)      # one round per chunk
    assert m_def.keys() == m_sh.keys() == m_sh5.keys() and all(math.isfinite(float(v)) for v in m_sh.values())
    # the per-candidate scores the default call ranks
    model = enc.bert_pretrained
    enc.eval()
    with torch.no_grad():
        base, _ = model.sequence_log_likelihood(s["input_ids"], s["image_feat"], s["image_loc"], s["masked_lm_labels"],
                                                token_type_ids=s["token_type_ids"], position_ids=s["token_position_ids"],
                                                attention_mask=s["attention_mask"], image_attention_mask=s["image_attention_mask"],
                                                co_attention_mask=s["co_attention_mask"])
    base = base.double().cpu().view(rounds, options)
    tol = 2e-3 * float(base.abs().max())
    for r in range(rounds):
        want = scores_to_ranks(base[r].view(1, 1, -1)).view(-1)
        rd, rs = r_def[0][0, r], r_sh[0][0, r]
        assert rd.tolist() == want.tolist()
        far = (base[r][:, None] - base[r][None, :]) > tol
        assert bool((rs[:, None] < rs[None, :])[far].all()), (r, rd.tolist(), rs.tolist(), base[r].tolist())
        assert sorted(rs.tolist()) == list(range(1, options + 1))
