"""Training-loop shell around the hot path: what train.py:350-507 does between the
dataloader and the checkpoint file, without the data plane.

* `train_step`       - one iteration of the loop body (train.py:411-463): forward through the harness, the
                       reference's loss combination, `/ batch_multiply`, backward, optimizer step + zero_grad
                       on accumulation boundaries only, scheduler step every iteration.  bf16 needs no
                       GradScaler; with the data-parallel wrapper the gradient exchange is skipped on
                       non-boundary micro-steps (`no_sync`).
* `save_checkpoint`  - the dict of train.py:503-505 (`model_state_dict` with the `bert_pretrained.` prefix,
                       `scheduler_state_dict`, `optimizer_state_dict`, `iter_id`).
* `load_checkpoint`  - warm start by key intersection (train.py:352-364) or `-continue` (train.py:366-389).
* `expand_image_fields` - train.py:413-432 (one image's features repeated per round and per sample).
* `dense_finetune_step` - one iteration of dense_annotation_finetuning.py:146-301 (row F4): one annotated
                       round of one image against its 100 options (ground truth first, the rest permuted),
                       NeuralNDCG^T + LM + weighted NSP objective, scheduler stepped before the optimizer.
* `self_critical_step` - one iteration of policy-gradient fine-tuning of the answer generator on a host-side
                       reward (an extension, unimm_amd/policy.py): sample answers, score them, train on the advantage.
* `distill_step`     - `train_step` with the LM term distilled from a frozen teacher (an extension, unimm_amd/policy.py).
* `visdial_evaluate`  - the validation pass of train.py:180-290 (chunked NSP scoring -> SparseGTMetrics + NDCG).
* `generative_evaluate` - the validation pass of val_lm.py:38-150 (candidates ranked by sequence log-likelihood)."""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import harness, metrics, ranking
from .policy import (DistillObjective, PolicyObjective, PreferenceObjective, PreferenceTargets, _pretraining_model, candidate_training_batch,
                     preference_diagnostics, sampled_training_batch, self_critical_advantage, spread)
from .reward import DeviceReward
from .scoring import SharedContext


def expand_image_fields(batch: dict) -> dict:
    """[n_img, ...] image tensors -> [n_img, rounds, samples, ...] as `forward` flattens them (train.py:413-432)."""
    rounds, samples = batch["tokens"].shape[1], batch["tokens"].shape[2]
    out = dict(batch)
    for k in ("image_feat", "image_loc", "image_target", "image_label", "image_mask"):
        if k not in batch:
            continue                          # evaluation batches carry no targets / labels
        v = batch[k]
        out[k] = v.unsqueeze(1).unsqueeze(1).expand(v.shape[0], rounds, samples, *v.shape[1:]).contiguous()
    return out


def train_step(dialog_encoder, optimizer, scheduler, batch, params, iter_id, sample_size=None, model_kw=None):
    """One loop iteration (iter_id is the 1-based counter of train.py:411).  Returns (loss, lm, nsp, img) floats.
    model_kw: further keywords of the encoder's call (`harness.forward`); None: the reference's step."""
    bm = int(params.get("batch_multiply", 1))
    boundary = iter_id % bm == 0
    dialog_encoder.train()
    sync_ctx = dialog_encoder.no_sync() if (hasattr(dialog_encoder, "no_sync") and not boundary) else _null()
    with sync_ctx:
        loss, lm_loss, nsp_loss, img_loss = harness.forward(dialog_encoder, batch, params, sample_size=sample_size, model_kw=model_kw)
        (loss / bm).backward()
    if boundary:
        if hasattr(dialog_encoder, "sync_gradients"):
            dialog_encoder.sync_gradients()           # no-op when every bucket was reduced inside backward
        optimizer.step()
        optimizer.zero_grad()
    scheduler.step()
    return float(loss.detach()), lm_loss, nsp_loss, img_loss


def distill_step(dialog_encoder, optimizer, scheduler, batch, params, iter_id, *, teacher, objective=DistillObjective(),
                 sample_size=None):
    """One iteration of token-level knowledge distillation (an extension, unimm_amd/policy.py): `train_step` on an ordinary
    training batch with the LM term replaced by `objective` against the frozen `teacher` (`lm_objective=objective`,
    `lm_reference=teacher`; the batch's `weights` still weigh the hard-label share).  The NSP and region terms train as usual, the
    `batch_multiply` / `no_sync` cadence is `train_step`'s.  The teacher may be deeper or wider than the student (a separate model
    in eval() with requires_grad_(False), or `policy.frozen_reference(model)`); nothing of it changes.  The step's mean
    KL(teacher || student) is in `engine.last_lm_distill` afterwards.  -> `train_step`'s tuple."""
    engine = _pretraining_model(_unwrap(dialog_encoder)).engine
    engine.last_lm_distill = None              # never a value an earlier step left behind
    return train_step(dialog_encoder, optimizer, scheduler, batch, params, iter_id, sample_size=sample_size,
                      model_kw=dict(lm_objective=objective, lm_reference=teacher))


_OPTION_FIELDS = ("tokens", "segments", "positions", "weights", "sep_indices", "mask", "hist_len",
                  "next_sentence_labels", "txt_attention_mask", "co_attention_mask")


def select_options(batch: dict, option_indices: torch.Tensor) -> dict:
    """Reorder / subsample the option axis (dim 2) of every per-option field
    (dense_annotation_finetuning.py:211-220)."""
    out = dict(batch)
    for k in _OPTION_FIELDS:
        out[k] = batch[k].index_select(2, option_indices.to(batch[k].device))
    return out


def dense_finetune_step(dialog_encoder, optimizer, scheduler, batch, params, iter_id, num_options=100, option_indices=None):
    """One dense-annotation iteration.  `batch` holds ONE image (dense_annotation_finetuning.py:159) with
    `tokens` [1, 1, 100, T], `gt_option` and `gt_relevance` [1, 100].  `option_indices` overrides the random
    draw (tests).  Returns (loss, parts) with parts = target / nsp / lm tensors."""
    if batch["image_feat"].shape[0] != 1:
        raise ValueError("dense fine-tuning takes one image per step")
    bm = int(params.get("batch_multiply", 1))
    dialog_encoder.train()
    if option_indices is None:
        gt = int(batch["gt_option"].item())
        n_all = batch["tokens"].shape[2]
        rest = torch.cat([torch.arange(gt), torch.arange(gt + 1, n_all)])[torch.randperm(n_all - 1)[:num_options - 1]]
        option_indices = torch.cat([batch["gt_option"].view(-1).cpu().long(), rest])
    sel = expand_image_fields(select_options(batch, option_indices))
    boundary = iter_id % bm == 0 and iter_id > 0
    sync_ctx = dialog_encoder.no_sync() if (hasattr(dialog_encoder, "no_sync") and not boundary) else _null()
    with sync_ctx:
        _, lm_loss, _, _, nsp_scores = harness.forward(dialog_encoder, sel, params, output_nsp_scores=True)
        dev = nsp_scores.device
        relevance = batch["gt_relevance"].to(dev)[:, option_indices.to(dev)]
        loss, parts = ranking.dense_finetune_loss(nsp_scores, sel["next_sentence_labels"].to(dev), relevance, lm_loss,
                                                  params["nsp_loss_coeff"], num_options=len(option_indices))
        (loss / bm).backward()
    scheduler.step()
    if boundary:
        if hasattr(dialog_encoder, "sync_gradients"):
            dialog_encoder.sync_gradients()
        optimizer.step()
        optimizer.zero_grad()
    return float(loss.detach()) / bm, {k: v.detach() for k, v in parts.items()}


def _lm_term_step(dialog_encoder, optimizer, scheduler, batch, params, iter_id, sb, shared_context, reports, **lm_kw):
    """What `self_critical_step` and `preference_step` do with their SampledBatch `sb`: the train-mode `forward_backward` on the
    LM term alone (loss_weights (1 / bm, 0, 0)) with the objective arguments `lm_kw`, then the `no_sync` / `sync_gradients` /
    optimizer cadence of `train_step`.  reports: the `engine.last_lm_*` attributes the step sets, cleared first (never a value
    an earlier step left behind).  The NSP and region terms still run and must stay finite: label 0 everywhere, one labelled
    region per sequence against a uniform target distribution.  -> (lm_loss, the engine)."""
    bm = int(params.get("batch_multiply", 1))
    boundary = iter_id % bm == 0
    K, (G, R) = sb.input_ids.shape[0], batch["image_feat"].shape[:2]
    engine = _pretraining_model(_unwrap(dialog_encoder)).engine
    image_label = torch.zeros((K, R), dtype=torch.int64)
    image_label[:, 0] = 1
    C = engine.cfg.v_target_size
    dialog_encoder.train()
    for name in reports:
        setattr(engine, name, None)
    sync_ctx = dialog_encoder.no_sync() if (hasattr(dialog_encoder, "no_sync") and not boundary) else _null()
    with sync_ctx:
        _, lm_loss, _, _, _ = dialog_encoder.forward_backward(
            sb.input_ids, batch["image_feat"], batch["image_loc"], (1.0 / bm, 0.0, 0.0), token_type_ids=sb.token_type_ids,
            token_position_ids=sb.position_ids, attention_mask=sb.attention_mask, masked_lm_labels=sb.masked_lm_labels,
            next_sentence_label=torch.zeros(K, dtype=torch.int64),
            image_attention_mask=batch["image_mask"][sb.image_index.to(batch["image_mask"].device)] if "image_mask" in batch else None,
            image_label=image_label, image_target=torch.full((G, R, C), 1.0 / C), image_index=sb.image_index,
            **(dict(shared_context=SharedContext(sb.image_index, 64)) if shared_context else {}), **lm_kw)
    if boundary:
        if hasattr(dialog_encoder, "sync_gradients"):
            dialog_encoder.sync_gradients()
        optimizer.step()
        optimizer.zero_grad()
    scheduler.step()
    return lm_loss, engine


def self_critical_step(dialog_encoder, optimizer, scheduler, batch, params, iter_id, reward_fn, *, samples, baseline="greedy",
                       objective=PolicyObjective(), temperature=1.0, top_k=0, top_p=1.0, max_answer_len=20, seed=None,
                       shared_context=False, rollout="separate", reference=None, no_repeat_ngram_size=0, repetition_penalty=1.0,
                       repeat_scope="answer", draft=None, draft_len=4):
    """One iteration of self-critical / policy-gradient training of the answer generator (unimm_amd/policy.py).
    `batch` holds G dialog contexts: `tokens` / `segments` / `positions` [G, T] with the context `[CLS] caption [SEP] ... q_r
    [SEP]` in the first `context_len[g]` positions, `image_feat` / `image_loc` [G, R, .] and optionally `image_mask` [G, R].
    The model draws `samples` answers per dialog in eval mode (and, for baseline="greedy", its greedy answer);
    `reward_fn(tokens [G, N, W], lengths [G, N]) -> rewards [G, N]` scores them on the host -- or, when `reward_fn` is a
    `reward.DeviceReward` (`reward.CiderD`), on the device against `batch["reference_tokens"]` [G, M, Wr] /
    `batch["reference_lengths"]` [G, M] / optionally `batch["reference_weights"]` [G, M] (ValueError before the rollout when a
    key is missing), samples and greedy baseline alike, and only the [G, N] rewards come to the host; the advantage (reward minus
    the greedy reward, minus the mean of the dialog's other samples for "mean", or the reward itself for None) weighs the
    `objective` on every token of its answer; mode "ratio" corrects for temperature / top-k / nucleus sampling with the
    tokens' step_logq.  The train-mode step is `forward_backward` on the LM term alone, with the `batch_multiply` /
    `no_sync` / `sync_gradients` cadence of `train_step`.  seed: of the draws (default iter_id).
    shared_context: the train-mode step computes each dialog's context and image once for its N answers, forward and backward
    (`forward_backward(shared_context=SharedContext(sb.image_index, 64))`): the same gradient up to summation order, less work.
    An answer then has at most 30 tokens (max_answer_len <= 30: its 1 + 2 (n + 1) private rows fit two 32-row tiles; ValueError
    otherwise).  A step whose sampled answers all have at most 14 tokens runs the one-tile launches, bit for bit.
    rollout: "separate" decodes the greedy baseline in a generate_answers call of its own (beams = 1); "fused" (baseline="greedy"
    only, samples <= 15; ValueError otherwise) decodes it as one more slot of the sampling call, `generate_answers(samples=N,
    greedy=True)`: one prefill and one walk over the decode steps for both.  Only the samples are trained on either way.
    no_repeat_ngram_size / repetition_penalty / repeat_scope: `generate_answers`' history rules, handed to the sampling call and to
    the baseline's call alike, so the samples and the greedy baseline decode under one rule on both rollouts (a penalty changes
    the distribution drawn from: mode "ratio" reads it from step_logq).
    draft / draft_len: a draft model for the rollout (`generate_answers(draft=...)`, off by default): the sampling call runs
    with draft_accept="rejection" -- the samples stay distributed exactly as the model's own draws, with the step_logp / step_logq
    the objective reads -- and the separate rollout's greedy call with draft_accept="match".  The history rules are refused then.
    reference: the frozen model `objective.kl_coef > 0` leashes the policy to (`policy.frozen_reference(model)`, taken before
    the fine-tune; passed on as `lm_reference`); the step's mean KL is then in `engine.last_lm_kl`.
    -> (loss, mean reward and mean baseline of the samples that were trained on, mean entropy of the trained rows'
    distributions; NaN when the step decoded no row)."""
    greedy_baseline = isinstance(baseline, str) and baseline == "greedy"
    if rollout not in ("separate", "fused"):
        raise ValueError(f"self_critical_step: rollout must be 'separate' or 'fused', got {rollout!r}")
    if rollout == "fused" and not greedy_baseline:
        raise ValueError(f"self_critical_step: rollout='fused' decodes the greedy baseline with the samples and needs "
                         f"baseline='greedy', got baseline = {baseline!r}")
    fused = rollout == "fused"
    if shared_context and max_answer_len > 30:
        raise ValueError(f"self_critical_step: shared_context trains answers of at most 30 tokens (64 private rows), got "
                         f"max_answer_len = {max_answer_len}")
    if isinstance(reward_fn, DeviceReward):
        missing = [k for k in ("reference_tokens", "reference_lengths") if k not in batch]
        if missing:
            raise ValueError(f"self_critical_step: a DeviceReward scores against the batch's references; batch lacks {missing}")
        refs = (batch["reference_tokens"], batch["reference_lengths"], batch.get("reference_weights"))

        def score(tokens, lengths):              # on the device, as the answers are; only the [G, N] rewards come to the host
            return reward_fn.score(tokens, lengths, *refs)
    else:
        def score(tokens, lengths):
            return reward_fn(tokens.cpu(), lengths.cpu())
    model = _unwrap(dialog_encoder)
    T = batch["tokens"].shape[1]
    gen_args = (batch["tokens"], batch["image_feat"], batch["image_loc"], batch["context_len"])
    gen_kw = dict(token_type_ids=batch["segments"], position_ids=batch["positions"], image_attention_mask=batch.get("image_mask"),
                  max_answer_len=max_answer_len, no_repeat_ngram_size=no_repeat_ngram_size, repetition_penalty=repetition_penalty,
                  repeat_scope=repeat_scope)
    spec = dict(draft=draft, draft_len=draft_len) if draft is not None else {}
    dialog_encoder.eval()
    answers = model.generate_answers(*gen_args, samples=samples, temperature=temperature, top_k=top_k, top_p=top_p,
                                     seed=iter_id if seed is None else seed, **(dict(greedy=True) if fused else {}),
                                     **(dict(spec, draft_accept="rejection") if spec else {}), **gen_kw)
    rewards = torch.as_tensor(score(answers.tokens, answers.lengths)).to("cpu", torch.float32)
    if greedy_baseline:
        greedy = answers.greedy if fused else model.generate_answers(*gen_args, beams=1, **spec, **gen_kw)
        base = torch.as_tensor(score(greedy.tokens, greedy.lengths)).to("cpu", torch.float32).reshape(-1)
    else:
        base = baseline
    advantage = self_critical_advantage(rewards, base)
    sb = sampled_training_batch(batch["tokens"], batch["segments"], batch["positions"], batch["context_len"], answers, T)
    if sb.input_ids.shape[0] == 0:
        raise ValueError("self_critical_step: every sampled answer has length 0, there is nothing to train on")
    lm_loss, engine = _lm_term_step(
        dialog_encoder, optimizer, scheduler, batch, params, iter_id, sb, shared_context, ("last_lm_entropy", "last_lm_kl"),
        lm_advantage=spread(advantage, sb), lm_objective=objective, lm_reference=reference,
        lm_behaviour_logp=spread(answers.step_logq, sb) if objective.mode == "ratio" else None)
    entropy = engine.last_lm_entropy
    trained = rewards.reshape(-1)[sb.kept], advantage.reshape(-1)[sb.kept]      # hypotheses of length 0 took no part
    return (float(lm_loss), float(trained[0].mean()), float((trained[0] - trained[1]).mean()),
            float(entropy) if entropy is not None else float("nan"))


def preference_step(dialog_encoder, optimizer, scheduler, batch, params, iter_id, *, objective=PreferenceObjective(), reference=None,
                    shared_context=True):
    """One iteration of preference training of the answer generator on GIVEN candidate answers (unimm_amd/policy.py).
    `batch` holds G dialog contexts as `self_critical_step` takes them (`tokens` / `segments` / `positions` [G, T],
    `context_len` [G], `image_feat` / `image_loc` [G, R, .], optionally `image_mask` [G, R]) and their candidates:
    `answer_tokens` [G, N, W] (tokens, then [SEP], zero-padded), `answer_lengths` [G, N] (0 = absent) and `targets` [G, N], the
    target weight of each candidate (`policy.pair_targets`, `policy.relevance_targets`).  The train-mode step is
    `forward_backward` on the LM term alone with `lm_preference` / `lm_objective=objective` / `lm_reference=reference`, with the
    `batch_multiply` / `no_sync` / `sync_gradients` cadence of `self_critical_step`.  shared_context: each dialog's context and
    image are computed once for its candidates (`SharedContext(sb.image_index, 64)`); a candidate then has at most 30 tokens
    before its [SEP] (ValueError beyond).
    -> (loss, share of the dialogs whose best-scored candidate carries the largest target weight, mean score margin of that
    candidate over the dialog's others: `policy.preference_diagnostics` of `engine.last_lm_preference`, read after the step)."""
    lengths = torch.as_tensor(batch["answer_lengths"]).to("cpu", torch.int64)
    if shared_context and lengths.numel() and int(lengths.max()) - 1 > 30:
        raise ValueError(f"preference_step: shared_context trains answers of at most 30 tokens (64 private rows), got a candidate "
                         f"of {int(lengths.max()) - 1}")
    sb = candidate_training_batch(batch["tokens"], batch["segments"], batch["positions"], batch["context_len"],
                                  batch["answer_tokens"], lengths, batch["tokens"].shape[1])
    if sb.input_ids.shape[0] == 0:
        raise ValueError("preference_step: every candidate has length 0, there is nothing to train on")
    weights = torch.as_tensor(batch["targets"]).to("cpu", torch.float32)
    if tuple(weights.shape) != tuple(sb.shape):
        raise ValueError(f"preference_step: targets must be [G, N] = {tuple(sb.shape)}, got {tuple(weights.shape)}")
    targets = PreferenceTargets(sb.image_index, weights.reshape(-1)[sb.kept])
    lm_loss, engine = _lm_term_step(dialog_encoder, optimizer, scheduler, batch, params, iter_id, sb, shared_context,
                                    ("last_lm_preference",), lm_preference=targets, lm_objective=objective, lm_reference=reference)
    report = engine.last_lm_preference
    accuracy, margin = preference_diagnostics(report["seq_score"], targets)
    return float(lm_loss), accuracy, margin


def eval_chunk_size(n_gpus: int) -> int:
    """Sequences per evaluation forward: the largest divisor-friendly size not above 500 * n_gpus / 2 (train.py:186-190)."""
    cap = 500 * (n_gpus / 2)
    sizes = [1, 2, 4, 5, 100, 1000, 200, 8, 10, 40, 50, 500, 20, 25, 250, 125]
    return min(sizes, key=lambda x: abs(x - cap) if x <= cap else float("inf"))


_EVAL_TEXT = (("tokens", 1), ("segments", 1), ("positions", 1), ("weights", 1), ("sep_indices", 1), ("mask", 1),
              ("hist_len", 0), ("txt_attention_mask", 2), ("co_attention_mask", 2))


def _evaluate(dataloader, params, eval_batch_size, dialog_encoder, chunk, score_chunk, collect_ranks=None, with_groups=False):
    """Shared loop of the two validation passes: flatten an image's (round, option) sequences, score them chunk by
    chunk with `score_chunk(item) -> [chunk] scores (higher = better answer)`, accumulate the retrieval metrics.
    with_groups: an item also carries `group`, the (image, round) index of each of its sequences."""
    sparse, ndcg = metrics.SparseGTMetrics(), metrics.NDCG()
    was_training = dialog_encoder.training
    dialog_encoder.eval()
    with torch.no_grad():
        for batch in dataloader:
            rounds, options = batch["tokens"].shape[1], batch["tokens"].shape[2]
            total = eval_batch_size * rounds * options
            if batch["tokens"].shape[0] != eval_batch_size or total % chunk:
                raise ValueError(f"evaluation batch of {batch['tokens'].shape[0]} images x {rounds} x {options} sequences "
                                 f"does not split into chunks of {chunk}")
            flat = {k: batch[k].reshape((-1,) + tuple(batch[k].shape[-keep:])) if keep else batch[k].reshape(-1)
                    for k, keep in _EVAL_TEXT}
            img = expand_image_fields({k: batch[k] for k in ("tokens", "image_feat", "image_loc", "image_mask")})
            for k in ("image_feat", "image_loc"):
                flat[k] = img[k].reshape((-1,) + tuple(img[k].shape[-2:]))
            flat["image_mask"] = img["image_mask"].reshape(-1, img["image_mask"].shape[-1])
            if with_groups:
                flat["group"] = torch.arange(total) // options
            scores = [score_chunk({k: v[lo:lo + chunk] for k, v in flat.items()}) for lo in range(0, total, chunk)]
            output = torch.cat(scores).view(eval_batch_size, rounds, options)
            dev = output.device
            sparse.observe(output, batch["gt_option_inds"].to(dev))
            rid = batch["round_id"].reshape(-1).to(dev).long()
            ndcg.observe(output[torch.arange(eval_batch_size, device=dev), rid - 1, :], batch["gt_relevance"].to(dev))
            if collect_ranks is not None:
                collect_ranks.append(harness.scores_to_ranks(output).cpu())
    if was_training:
        dialog_encoder.train()
    out = sparse.retrieve(reset=True)
    out.update(ndcg.retrieve(reset=True))
    return out


def visdial_evaluate(dataloader, params, eval_batch_size, dialog_encoder, chunk_size=None):
    """Discriminative evaluation over a validation loader (train.py:180-290): every (round, option) sequence of
    each image is scored in chunks with the NSP head, P(option is the answer) is ranked against the ground-truth
    option (R@k, mean rank, MRR) and, on the densely annotated round, against the relevance scores (NDCG).
    Batches hold `tokens` [eval_batch_size, rounds, options, T], `gt_option_inds`, `gt_relevance`, `round_id`."""
    chunk = int(chunk_size or eval_chunk_size(int(params.get("n_gpus", 1))))

    def score(item):
        nsp_scores = harness.forward(dialog_encoder, item, params, output_nsp_scores=True, evaluation=True)[4]
        return torch.softmax(nsp_scores.float(), dim=1)[:, 0]

    return _evaluate(dataloader, params, eval_batch_size, dialog_encoder, chunk, score)


def generative_evaluate(dataloader, params, eval_batch_size, dialog_encoder, chunk_size=None, average=False, ranks_out=None,
                        shared_context=False):
    """Generative evaluation (val_lm.py:38-150; token-mean variant val_avg_lm.py:135 with average=True): every
    candidate answer is scored by the sum of its tokens' log-likelihoods under the masked-LM head, the candidates of a
    round are ranked by that score.  The reference decodes all 256 rows of every sequence into [chunk, 256, 30522]
    logits and cross-entropies them; here only the labelled rows are decoded (`sequence_log_likelihood`).  Chunks of
    `250 * n_gpus / 2` rounded down to the reference's size table (val_lm.py:47-49).  `ranks_out`: optional list that
    receives the [eval_batch_size, rounds, options] rank tensors (what val_lm.py:139-149 writes to its json).
    shared_context: score a chunk with the context and image of every (image, round) computed once for its candidates
    (`sequence_log_likelihood(shared_context=SharedContext(group, 64))`): the same scores up to the summation order inside the
    attention kernels.  A chunk that holds a candidate of more than 30 tokens is scored per candidate, as without the option."""
    if chunk_size is None:
        cap = 250 * (int(params.get("n_gpus", 1)) / 2)
        sizes = [1, 2, 4, 5, 100, 1000, 200, 8, 10, 40, 50, 500, 20, 25, 250, 125]
        chunk_size = min(sizes, key=lambda x: abs(x - cap) if x <= cap else float("inf"))
    model = _unwrap(dialog_encoder).bert_pretrained

    def score(item):
        shared = {}
        if shared_context and int((item["mask"] != -1).sum(-1).max()) <= 31:       # labelled rows = candidate tokens + [SEP]
            shared = dict(shared_context=SharedContext(item["group"], 64))
        s, _ = model.sequence_log_likelihood(
            item["tokens"], item["image_feat"], item["image_loc"], item["mask"], average=average,
            token_type_ids=item["segments"], position_ids=item["positions"], attention_mask=item["txt_attention_mask"],
            image_attention_mask=item["image_mask"], co_attention_mask=item["co_attention_mask"], **shared)
        return s

    return _evaluate(dataloader, params, eval_batch_size, dialog_encoder, int(chunk_size), score, collect_ranks=ranks_out,
                     with_groups=bool(shared_context))


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _unwrap(m):
    return m.module if hasattr(m, "module") else m


def save_checkpoint(path, dialog_encoder, optimizer, scheduler, iter_id):
    torch.save({"model_state_dict": _unwrap(dialog_encoder).state_dict(), "scheduler_state_dict": scheduler.state_dict(),
                "optimizer_state_dict": optimizer.state_dict(), "iter_id": iter_id}, path)
    return path


def load_checkpoint(path_or_dict, dialog_encoder, optimizer=None, scheduler=None, resume=False):
    """resume=False: copy every tensor whose key exists in the model (accepts a bare state_dict or the
    training dict); returns the number of keys transferred.  resume=True: also restore optimizer and
    scheduler state and return the saved iter_id."""
    ck = torch.load(path_or_dict, map_location="cpu") if isinstance(path_or_dict, (str, os.PathLike)) else path_or_dict
    model = _unwrap(dialog_encoder)
    model_dict = model.state_dict()
    if not resume:
        sd = ck["model_state_dict"] if "model_state_dict" in ck else ck
        sd = {k: v for k, v in sd.items() if k in model_dict}
        if not sd:
            raise ValueError("load_checkpoint: no key of the checkpoint exists in the model")
        model_dict.update(sd)
        model.load_state_dict(model_dict)
        return len(sd)
    model_dict.update({k: v for k, v in ck["model_state_dict"].items() if k in model_dict})
    model.load_state_dict(model_dict)
    if optimizer is not None:
        optimizer.load_state_dict(ck["optimizer_state_dict"])
    if scheduler is not None:
        scheduler.load_state_dict(ck["scheduler_state_dict"])
    return ck["iter_id"]
