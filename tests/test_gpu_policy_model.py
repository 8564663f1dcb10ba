"""The policy-gradient objective through the engine, the model surface and trainer.self_critical_step, on the small
configuration of tests/test_gpu_generate.py: bit-equality with the weighted-likelihood step for integer advantages, the
assembled batch against the sampler's own log p, the direction of one gradient step, the loop body end to end, the refusals on
the device and the graph executor's eager path."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_generate import gen_kwargs, make_dialogs, tiny  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "small_config.json")
T_TINY, G_TINY, MAXLEN = 64, 6, 8


def fresh(compute="bf16"):
    """A model of its own for the tests that change parameters (the weights of the `tiny` fixture)."""
    from oracle import vilbert_ref as R
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    cfgd = json.load(open(CFG))
    model = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd), compute_dtype=compute)
    sd = R.init_state_dict(R.make_config(cfgd), seed=11)
    sd["cls.predictions.bias"] = torch.randn(sd["cls.predictions.bias"].shape, generator=torch.Generator().manual_seed(5)) * 3.0
    model.load_state_dict(sd, strict=True)
    return model.cuda()


def tiny_dialogs(G=G_TINY, seed=21):
    return make_dialogs(G, T_TINY, 1000, 37, 192, seed=seed, cmin=8, cmax=40)


def train_kwargs(b, **more):
    kw = dict(token_type_ids=b["token_type_ids"], position_ids=b["token_position_ids"], attention_mask=b["attention_mask"],
              image_attention_mask=b["image_attention_mask"], co_attention_mask=b["co_attention_mask"],
              masked_lm_labels=b["masked_lm_labels"], image_label=b["image_label"], image_target=b["image_target"],
              next_sentence_label=b["next_sentence_label"], nsp_weight=b["nsp_weight"])
    kw.update(more)
    return kw


def step(model, b, seed, **more):
    """one forward_backward from zeroed gradients under a fixed dropout seed and step -> (losses, gradient arena)"""
    model.train()
    model.engine.ensure(torch.device("cuda", 0))
    model.set_dropout_seed(seed, 0)
    model.engine.arena.zero_grads()
    loss, lm, img, nsp, _ = model.forward_backward(b["input_ids"], b["image_feat"], b["image_loc"], (1.0, 0.5, 2.0),
                                                   **train_kwargs(b, **more))
    torch.cuda.synchronize()
    return torch.stack([loss.reshape(()), lm.reshape(()), img.reshape(()), nsp.reshape(())]).clone(), model.engine.arena.grad_flat.clone()


def weight_map(labels):
    """1 and 3 alternating on the labelled rows, 0 elsewhere"""
    flat = labels.reshape(-1)
    w = torch.zeros_like(flat)
    idx = torch.nonzero(flat != -1)[:, 0]
    w[idx] = torch.where(torch.arange(len(idx), device=idx.device) % 2 == 0, 1, 3).to(w.dtype)
    return w.view_as(labels)


def test_integer_advantage_equals_weighted_likelihood_bit_for_bit():
    """mode "logp", beta = 0, advantage = an integer weight map (1 and 3 on the labelled rows), same dropout seed and step as a
    step with lm_weight set to that map.  Bit for bit equal, unconditionally: the four losses, and the LM head's gradient -- the
    bf16 [rows, vocabulary] matrix `_lm_loss_grad` hands to the decoder's backward, the one thing the new kernels produce that
    the backward reads.  Every launch behind it is the weighted step's, on bit-identical operands.
    The gradient arena, bucket by bucket: a bucket on which three runs of the SAME weighted step agree bit for bit must be
    bit-equal in the policy step too.  On an MI355X that is every bucket but `text_embeddings`, whose word-embedding rows
    collect fp32 atomic adds (the embedding backward, on top of the tied decoder's gradient) in an order that differs from
    run to run.  On such a bucket the policy run is one more draw from the same distribution (identical operands, identical
    launches); the largest difference of a fourth exchangeable draw exceeds the largest of three pairwise differences in a
    fixed share of runs whatever the code does, so a gate of 1x the spread would fail at random: it is held to 2x the spread
    of the three weighted runs on that bucket.  A wrong coefficient cannot hide behind that: it is caught above, bit for bit."""
    from unimm_amd import synth
    from unimm_amd.policy import PolicyObjective
    model = fresh()
    b = synth.make_batch(n_seq=12, T=64, R=37, cfg=model.config, seed=5, device="cuda")
    w = weight_map(b["masked_lm_labels"])
    assert int((w == 1).sum()) > 3 and int((w == 3).sum()) > 3
    model.engine.ensure(torch.device("cuda", 0))
    head_grads, inner = [], model.engine._lm_loss_grad

    def spy(lm, g_lm):
        head_grads.append(inner(lm, g_lm).clone())
        return head_grads[-1]

    model.engine._lm_loss_grad = spy
    old = [step(model, b, 321, lm_weight=w) for _ in range(3)]
    new = step(model, b, 321, lm_advantage=w.float(), lm_objective=PolicyObjective(mode="logp", entropy_coef=0.0))
    assert len(head_grads) == 4 and head_grads[0].dtype == torch.bfloat16 and bool((head_grads[0] != 0).any())
    assert torch.isfinite(new[0]).all() and torch.isfinite(new[1]).all()
    assert torch.equal(new[0].view(torch.int32), old[0][0].view(torch.int32)), (new[0], old[0][0])     # loss, lm, img, nsp
    for i in (1, 2, 3):                      # the weighted step's own LM-head gradient is reproducible, the policy step's equals it
        assert torch.equal(head_grads[i].view(torch.int16), head_grads[0].view(torch.int16)), i
    noisy = []
    for name, lo, hi in model.engine.arena.used_ranges():
        o = [r[1][lo:hi] for r in old]
        spread = max(float((o[i] - o[j]).abs().max()) for i, j in ((0, 1), (0, 2), (1, 2)))
        if spread == 0.0:
            assert torch.equal(new[1][lo:hi].view(torch.int32), o[0].view(torch.int32)), name
        else:
            d = float((new[1][lo:hi] - o[0]).abs().max())
            noisy.append(f"{name}: |policy - weighted| max {d:.3e}, spread of three weighted runs {spread:.3e}, "
                         f"largest gradient {float(o[0].abs().max()):.3e}")
            assert d <= 2 * spread, noisy[-1]
    print(f"\ngradient arena: {len(model.engine.arena.used_ranges()) - len(noisy)} buckets bit-equal; not reproducible in the "
          f"weighted step itself: {noisy}")
    assert len(noisy) < len(model.engine.arena.used_ranges())


def test_assembled_batch_scores_equal_sampled_logp(tiny):
    """sequence_log_likelihood of sampled_training_batch(...) equals the sampler's logp: |difference| <= 2e-3 of the largest
    |score|, the gate of tests/test_gpu_generate_sample.py for the same identity."""
    from unimm_amd.policy import sampled_training_batch
    model, _, _ = tiny
    d, c, _ = tiny_dialogs()
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, samples=4, max_answer_len=MAXLEN, top_p=0.9,
                                 temperature=0.8, seed=2, **gen_kwargs(d))
    sb = sampled_training_batch(d["input_ids"], d["token_type_ids"], d["position_ids"], c, res, T_TINY)
    assert sb.input_ids.shape[0] == G_TINY * 4
    dev = "cuda"
    want, _ = model.sequence_log_likelihood(sb.input_ids.to(dev), d["image_feat"].to(dev), d["image_loc"].to(dev),
                                            sb.masked_lm_labels.to(dev), token_type_ids=sb.token_type_ids.to(dev),
                                            position_ids=sb.position_ids.to(dev), attention_mask=sb.attention_mask,
                                            image_attention_mask=d["image_attention_mask"][sb.image_index].to(dev),
                                            image_index=sb.image_index.to(dev))
    got, want = res.logp.reshape(-1)[sb.kept.to(res.logp.device)].cpu(), want.cpu()
    scale, err = float(want.abs().max()), float((got - want).abs().max())
    print(f"\nlogp {float(got.min()):.3f} .. {float(got.max()):.3f}: |sampled - assembled| {err:.3e} ({err / scale:.2e} of scale)")
    assert err <= 2e-3 * scale


def seq_logp(model, sb, d):
    model.eval()
    dev = "cuda"
    s, _ = model.sequence_log_likelihood(sb.input_ids.to(dev), d["image_feat"].to(dev), d["image_loc"].to(dev),
                                         sb.masked_lm_labels.to(dev), token_type_ids=sb.token_type_ids.to(dev),
                                         position_ids=sb.position_ids.to(dev), attention_mask=sb.attention_mask,
                                         image_attention_mask=d["image_attention_mask"][sb.image_index].to(dev),
                                         image_index=sb.image_index.to(dev))
    return s.double().cpu()


def policy_inputs(sb, d, G, C):
    """the inputs `self_critical_step` builds around a SampledBatch"""
    K, R = sb.input_ids.shape[0], d["image_feat"].shape[1]
    label = torch.zeros((K, R), dtype=torch.int64)
    label[:, 0] = 1
    return dict(token_type_ids=sb.token_type_ids, position_ids=sb.position_ids, attention_mask=sb.attention_mask,
                masked_lm_labels=sb.masked_lm_labels, next_sentence_label=torch.zeros(K, dtype=torch.int64),
                image_attention_mask=d["image_attention_mask"][sb.image_index], image_label=label,
                image_target=torch.full((G, R, C), 1.0 / C), image_index=sb.image_index)


DIRECTION_SEED, DIRECTION_LR = 3, 1e-2


def test_one_gradient_step_moves_the_samples_apart():
    """Two samples of one dialog with advantages +1 and -1, one plain step p -= lr grad: in eval mode the log-likelihood of the
    first rises and of the second falls."""
    from unimm_amd.policy import sampled_training_batch, spread
    model = fresh().eval()
    d, c, _ = tiny_dialogs(G=1)
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, samples=2, max_answer_len=MAXLEN,
                                 seed=DIRECTION_SEED, **gen_kwargs(d))
    assert not torch.equal(res.tokens[0, 0], res.tokens[0, 1]), "the two samples must differ"
    sb = sampled_training_batch(d["input_ids"], d["token_type_ids"], d["position_ids"], c, res, T_TINY)
    before = seq_logp(model, sb, d)
    kw = policy_inputs(sb, d, 1, model.config.v_target_size)
    model.train()
    model.set_dropout_seed(7, 0)
    model.engine.arena.zero_grads()                      # (the arena exists: the eval passes above ran on it)
    model.forward_backward(sb.input_ids, d["image_feat"], d["image_loc"], (1.0, 0.0, 0.0),
                           lm_advantage=spread(torch.tensor([[1.0, -1.0]]), sb), **kw)
    with torch.no_grad():
        model.engine.arena.flat.sub_(DIRECTION_LR * model.engine.arena.grad_flat)
    model.engine.invalidate_weights()
    after = seq_logp(model, sb, d)
    print(f"\nlog-likelihood of the +1 sample {before[0]:.4f} -> {after[0]:.4f}, of the -1 sample {before[1]:.4f} -> {after[1]:.4f}")
    assert after[0] > before[0] and after[1] < before[1]


def _encoder():
    from unimm_amd import VisualDialogEncoder
    from unimm_amd.optim import FusedAdamW, WarmupLinearScheduleNonZero, default_language_weights, reference_param_groups
    torch.manual_seed(5)
    enc = VisualDialogEncoder(CFG).to("cuda")
    groups = reference_param_groups(enc, lr=1e-3, image_lr=4e-3, language_weights=default_language_weights(enc))
    opt = FusedAdamW(groups, enc.bert_pretrained.engine, lr=1e-3)
    return enc, opt, WarmupLinearScheduleNonZero(opt, warmup_steps=2, t_total=20, min_lr=1e-5)


@pytest.mark.parametrize("baseline,objective_kw,sample_kw", [
    ("greedy", dict(), dict()),
    ("mean", dict(entropy_coef=0.01), dict()),
    ("mean", dict(mode="ratio", clip_eps=0.2, entropy_coef=0.01), dict(top_k=20, temperature=0.8)),
])
def test_self_critical_step_end_to_end(baseline, objective_kw, sample_kw):
    from unimm_amd import trainer
    from unimm_amd.policy import PolicyObjective
    enc, opt, sch = _encoder()
    d, c, _ = tiny_dialogs(G=4, seed=8)
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"])
    eng = enc.bert_pretrained.engine
    eng.ensure(torch.device("cuda", 0))
    p0 = eng.arena.flat.clone()
    reward = lambda tokens, lengths: -lengths.float()                  # toy host reward: shorter answers are better
    out = trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), 1, reward, samples=3, baseline=baseline,
                                     objective=PolicyObjective(**objective_kw), max_answer_len=MAXLEN, seed=4, **sample_kw)
    torch.cuda.synchronize()
    loss, mean_reward, mean_baseline, mean_entropy = out
    print(f"\nself_critical_step({baseline}, {objective_kw}): loss {loss:.4f} reward {mean_reward:.3f} baseline {mean_baseline:.3f} "
          f"entropy {mean_entropy:.4f}")
    assert all(math.isfinite(v) for v in out)
    assert mean_entropy > 0 and -MAXLEN - 1 <= mean_reward <= -1
    assert enc.training
    assert not torch.equal(p0, eng.arena.flat), "the optimizer stepped"
    assert torch.isfinite(eng.arena.flat).all()


def test_refusals_on_the_device():
    from unimm_amd import synth
    m = fresh()
    b = synth.make_batch(n_seq=6, T=64, R=37, cfg=m.config, seed=3, device="cuda")
    adv = torch.ones((6, 64), device="cuda")
    with pytest.raises(ValueError, match="pass one of them"):
        m.forward_backward(b["input_ids"], b["image_feat"], b["image_loc"], (1.0, 1.0, 1.0),
                           **train_kwargs(b, lm_weight=b["lm_weight"], lm_advantage=adv))
    x3 = fresh("fp32x3")
    with pytest.raises(ValueError, match="bf16 engine only"):
        x3.forward_backward(b["input_ids"], b["image_feat"], b["image_loc"], (1.0, 1.0, 1.0), **train_kwargs(b, lm_advantage=adv))
    with pytest.raises(ValueError, match="bf16 engine only"):
        x3(b["input_ids"], b["image_feat"], b["image_loc"], **train_kwargs(b, lm_advantage=adv))


def test_graph_executor_takes_the_eager_path():
    """With the step executor enabled the policy step is not eligible: nothing is captured or replayed, and the losses equal
    those of a model without it (2e-6, the gate of tests/test_gpu_graphs.py for the same comparison)."""
    from unimm_amd import synth
    from unimm_amd.policy import PolicyObjective
    ref, gm = fresh(), fresh()
    b = synth.make_batch(n_seq=12, T=64, R=37, cfg=ref.config, seed=5, device="cuda")
    rng = torch.Generator().manual_seed(1)
    adv = torch.randn((12, 64), generator=rng).cuda()
    blogp = (-3.0 + torch.randn((12, 64), generator=rng)).cuda()
    obj = PolicyObjective(mode="ratio", clip_eps=0.2, entropy_coef=0.01)
    gm.engine.ensure(torch.device("cuda", 0))
    graphs = gm.engine.enable_graphs(row_bucket=64, lm_bucket=16, capture_after=0)
    for i in range(3):
        want, _ = step(ref, b, 55 + i, lm_advantage=adv, lm_behaviour_logp=blogp, lm_objective=obj)
        got, _ = step(gm, b, 55 + i, lm_advantage=adv, lm_behaviour_logp=blogp, lm_objective=obj)
        assert torch.isfinite(got).all()
        assert (want - got).abs().max() <= 2e-6 * max(1.0, float(want.abs().max())), (i, want, got)
    assert graphs.stats["replays"] == 0 and graphs.stats["captures"] == 0, graphs.stats
    # the likelihood step on the same model is still replayed
    step(gm, b, 60, lm_weight=b["lm_weight"])
    step(gm, b, 61, lm_weight=b["lm_weight"])
    assert graphs.stats["captures"] >= 1, graphs.stats
