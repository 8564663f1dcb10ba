"""Policy-gradient fine-tuning of the answer generator on a sequence-level reward (an extension; the reference trains the
generative head by likelihood only).

`generate_answers(samples=N)` draws N answers per dialog and returns, per token, log p under the model (step_logp) and log q
under the distribution it was drawn from (step_logq).  A host-side reward (NDCG of the answer, an answer-quality metric, a
preference score) turns into a per-sequence advantage, and the LM head's objective on the [MASK]-copy rows of the sampled
sequences becomes (csrc/policy.hip, include/unimm_hip.h: unimm_pg_loss_fwd / _bwd)

    mode "logp"    -A log p_y                                              REINFORCE / self-critical
    mode "ratio"   -min(r A, clamp(r, 1 - clip_eps, 1 + clip_eps) A)       r = p_y / q_y; clip_eps = inf: importance-weighted
    both           -entropy_coef H(p)                                      entropy bonus of the row's distribution
    both           +kl_coef KL(p || p_ref)                                 leash on a frozen reference model (kl_coef > 0)

summed over the labelled rows and divided by their number, exactly where the weighted likelihood sits otherwise: the row-sparse
decoder, the transform head's backward, the weight-gradient ledger and the data-parallel buckets are the training step's.

This module is host-side: the objective's description, the refusals, the assembly of the training batch from the sampled
answers (the layout `utils/data_utils.py:139-288` gives a generative sequence; `oracle/masks.py::encode_gen` restates it) and the
advantage arithmetic.  The data is small and on the host anyway, where the reward is computed.  `trainer.self_critical_step`
is the loop body.

The KL leash (unimm_pg_kl_loss_fwd / _bwd): `lm_reference=frozen_reference(model)`, taken before the fine-tune starts, with
`PolicyObjective(kl_coef=c)`.  Every step the reference's engine first runs an inference forward on the step's own inputs and
hands over its fp32 logits for exactly the step's decoded rows; the row kernels stream them beside the policy's and add the
EXACT full-vocabulary c KL(p || p_ref) per row and its gradient (not the sampled estimate log p_y - log p_ref,y).  Nothing
of the reference changes; `engine.last_lm_kl` reports the mean KL of the trained rows beside `engine.last_lm_entropy`.

Preference training (unimm_seq_pref): instead of a reward on answers the model sampled, GIVEN candidate answers with target
weights -- a chosen and a rejected answer, or the 100 options of a round with their dense relevance annotations.
`candidate_training_batch` lays the candidates out as `sampled_training_batch` lays out samples, `lm_preference=
PreferenceTargets(group, weight)` names each sequence's dialog and target weight, and `lm_objective=PreferenceObjective(beta,
length_normalize)` makes lm_loss, per dialog, the cross-entropy between the targets and the softmax over the dialog's candidates
of beta (log pi(y) - log pi_ref(y)) (divided by the answer's length with length_normalize): DPO for two candidates and a one-hot
target (`pair_targets`), the listwise ListNet top-1 form for `relevance_targets`, on exactly the scores `generative_evaluate`
ranks by.  `lm_reference` is optional (without one log pi_ref = 0).  `trainer.preference_step` is the loop body.

Knowledge distillation (unimm_distill_loss_fwd / _bwd, csrc/distill.hip): a student fits a frozen teacher's softened distribution
on ordinary training data.  `lm_reference=teacher` with `lm_objective=DistillObjective(temperature, alpha)` makes the LM loss of
every labelled row
    alpha (the weighted likelihood / unlikelihood, `lm_weight` as ever) + (1 - alpha) tau^2 KL(softmax(zr / tau) || softmax(z / tau))
with the teacher's logits zr for the same rows (`Engine._reference_rows`, as for the KL leash) -- the other direction of KL, a
temperature, and no advantage.  The teacher need not have the student's shape (`check_teacher`): any depth, width, head count or
layer schedule over the same vocabulary and inputs, typically a larger model in eval() with requires_grad_(False);
`frozen_reference(model)` serves self-distillation.  `engine.last_lm_distill` reports the mean KL of the trained rows;
`trainer.distill_step` is the loop body."""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import lm_objective as LO
from .inputs import DialogMaskSpec

SEP, MASK = 102, 103


@dataclass(frozen=True)
class PolicyObjective:
    """mode: "logp" | "ratio"; clip_eps: the ratio's clipping range (inf = none); entropy_coef: weight of the entropy bonus;
    kl_coef: weight of the per-row KL(p || p_ref) against the frozen `lm_reference` (0 = none, the reference is then ignored)."""
    mode: str = "logp"
    clip_eps: float = math.inf
    entropy_coef: float = 0.0
    kl_coef: float = 0.0

    def __post_init__(self):
        if self.mode not in ("logp", "ratio"):
            raise ValueError(f"PolicyObjective: mode must be 'logp' or 'ratio', got {self.mode!r}")
        if not float(self.clip_eps) >= 0.0:
            raise ValueError(f"PolicyObjective: clip_eps must be >= 0 (inf = no clipping), got {self.clip_eps}")
        if not math.isfinite(float(self.entropy_coef)):
            raise ValueError(f"PolicyObjective: entropy_coef must be finite, got {self.entropy_coef}")
        if not (math.isfinite(float(self.kl_coef)) and float(self.kl_coef) >= 0.0):
            raise ValueError(f"PolicyObjective: kl_coef must be finite and >= 0, got {self.kl_coef}")


@dataclass(frozen=True)
class PreferenceObjective:
    """beta: the temperature of the comparison, z = beta (log pi(y) - log pi_ref(y)); length_normalize: divide a candidate's
    score by its number of decoded rows (the mean val_avg_lm.py ranks by) instead of taking the sum (val_lm.py)."""
    beta: float = 0.1
    length_normalize: bool = False

    def __post_init__(self):
        b = float(self.beta)
        if not (math.isfinite(b) and b > 0.0):
            raise ValueError(f"PreferenceObjective: beta must be positive and finite, got {self.beta}")


@dataclass(frozen=True)
class DistillObjective:
    """temperature: tau > 0, both distributions are softmax(logits / tau); alpha: the share of the hard-label term (the weighted
    likelihood of the labels) in [0, 1], the soft term tau^2 KL(teacher || student) has 1 - alpha (1: the teacher is not run)."""
    temperature: float = 2.0
    alpha: float = 0.5

    def __post_init__(self):
        _check_distill_values(self.temperature, self.alpha)


def _check_distill_values(temperature, alpha):
    try:
        t, a = float(temperature), float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"DistillObjective: temperature and alpha must be numbers, got {temperature!r} / {alpha!r}") from None
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"DistillObjective: temperature must be positive and finite, got {temperature}")
    if not 0.0 <= a <= 1.0:
        raise ValueError(f"DistillObjective: alpha must lie in [0, 1], got {alpha}")


PREF_MAX_MEMBERS = 128        # include/unimm_hip.h: UNIMM_PREF_MAX_MEMBERS


class PreferenceTargets:
    """One group id (the sequence's dialog, an integer >= 0) and one target weight >= 0 per sequence of the step; host data.
    A group whose weights sum to 0 takes no part in the step."""

    def __init__(self, group, weight):
        g = np.asarray(group.detach().cpu() if torch.is_tensor(group) else group)
        w = np.asarray(weight.detach().cpu() if torch.is_tensor(weight) else weight)
        if g.ndim != 1 or w.ndim != 1 or (g.size and not np.issubdtype(g.dtype, np.integer)):
            raise ValueError(f"PreferenceTargets: group must be a 1-D integer array and weight a 1-D array (one entry per sequence), "
                             f"got shapes {g.shape} / {w.shape}, group dtype {g.dtype}")
        self.group = g.astype(np.int64)
        self.weight = w.astype(np.float32)

    @property
    def groups(self):
        """number of group slots: the largest id + 1"""
        return int(self.group.max()) + 1 if self.group.size else 0

    def __len__(self):
        return int(self.group.shape[0])


def relevance_targets(gt_relevance, temperature=1.0):
    """Dense relevance annotations [G, N] -> the row-wise softmax(relevance / temperature), fp32 [G, N] (host)."""
    r = torch.as_tensor(gt_relevance).detach().to("cpu", torch.float32)
    if r.dim() != 2:
        raise ValueError(f"relevance_targets: gt_relevance must be [G, N], got {tuple(r.shape)}")
    if not (math.isfinite(float(temperature)) and float(temperature) > 0.0):
        raise ValueError(f"relevance_targets: temperature must be positive and finite, got {temperature}")
    return torch.softmax(r / float(temperature), dim=1)


def pair_targets(chosen, N):
    """chosen [G] (the index of the preferred candidate of each dialog) -> the one-hot rows, fp32 [G, N] (host)."""
    c = torch.as_tensor(chosen).detach().to("cpu", torch.int64).reshape(-1)
    N = int(N)
    if N < 1 or (c.numel() and (int(c.min()) < 0 or int(c.max()) >= N)):
        raise ValueError(f"pair_targets: every chosen index must lie in [0, N = {N})")
    out = torch.zeros((c.shape[0], N), dtype=torch.float32)
    out[torch.arange(c.shape[0]), c] = 1.0
    return out


def check_preference_inputs(shape, lm_preference, lm_objective, lm_advantage, lm_weight, lm_behaviour_logp, compute_dtype,
                            train_branch=True):
    """The refused combinations of the preference arguments of `forward` / `forward_backward` (ValueError, before anything
    touches the device) -> the objective in force.  `check_reference` judges the reference."""
    for name, t in (("lm_advantage", lm_advantage), ("lm_weight", lm_weight), ("lm_behaviour_logp", lm_behaviour_logp)):
        if t is not None:
            raise ValueError(f"lm_preference (the preference objective over whole answers) and {name} describe two objectives "
                             "for the same rows: pass one of them")
    if isinstance(lm_objective, PolicyObjective):
        raise ValueError("lm_preference takes a policy.PreferenceObjective; a PolicyObjective weighs lm_advantage")
    if not isinstance(lm_objective, PreferenceObjective):
        got = "None" if lm_objective is None else type(lm_objective).__name__
        raise ValueError(f"lm_preference needs lm_objective=policy.PreferenceObjective(...), got {got}")
    if not isinstance(lm_preference, PreferenceTargets):
        raise ValueError(f"lm_preference must be a policy.PreferenceTargets, got {type(lm_preference).__name__}")
    if compute_dtype != "bf16":
        raise ValueError(f"the preference objective runs on the bf16 engine only: build the model with compute_dtype='bf16' "
                         f"(got {compute_dtype!r})")
    b = float(lm_objective.beta)
    if not (math.isfinite(b) and b > 0.0):
        raise ValueError(f"PreferenceObjective: beta must be positive and finite, got {lm_objective.beta}")
    B = int(shape[0])
    g, w = lm_preference.group, lm_preference.weight
    if g.shape[0] != B or w.shape[0] != B:
        raise ValueError(f"lm_preference holds {g.shape[0]} group ids and {w.shape[0]} weights for {B} sequences: one of each per "
                         "sequence")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("lm_preference: every target weight must be finite and >= 0")
    if np.any(g < 0) or np.any(g >= 2 ** 31 - 1):
        raise ValueError("lm_preference: every group id must be an integer >= 0")
    if B and int(np.bincount(g).max()) > PREF_MAX_MEMBERS:
        raise ValueError(f"lm_preference: a group has {int(np.bincount(g).max())} sequences, at most {PREF_MAX_MEMBERS} can be "
                         "compared with each other")
    if not train_branch:
        raise ValueError("lm_preference replaces the LM loss of the train branch: pass masked_lm_labels, next_sentence_label and "
                         "image_target with it (this call computes no loss and would ignore it)")
    return lm_objective


def preference_diagnostics(seq_score, targets):
    """Two host-side figures of a preference step from its per-sequence scores D (`engine.last_lm_preference["seq_score"]`, NaN
    for a sequence without rows) and its `PreferenceTargets`, each a mean over the groups that took part (target weights
    summing to > 0 over the members that have rows): whether the best-scored member is the one with the group's largest weight
    (the first such member on ties), and D of that member minus the mean D of the group's other members, weighted by their
    target weights (plainly when those are all 0, as the rejected answer's is).  -> (accuracy, margin); NaN without a group."""
    D = np.asarray(seq_score.detach().cpu() if torch.is_tensor(seq_score) else seq_score, dtype=np.float64).reshape(-1)
    hit, margin = [], []
    for g in np.unique(targets.group):
        mem = [j for j in np.flatnonzero(targets.group == g) if not math.isnan(D[j])]
        w = targets.weight[mem].astype(np.float64)
        if not mem or not w.sum() > 0:
            continue
        top = int(np.argmax(w))
        hit.append(1.0 if int(np.argmax(D[mem])) == top else 0.0)
        others = [k for k in range(len(mem)) if k != top]
        if others:
            wo = w[others] if w[others].sum() > 0 else np.ones(len(others))
            margin.append(D[mem[top]] - float((wo * D[mem][others]).sum() / wo.sum()))
    mean = lambda v: float(np.mean(v)) if v else float("nan")
    return mean(hit), mean(margin)


def _pretraining_model(model):
    """a VisualDialogEncoder or a BertForMultiModalPreTraining -> the latter"""
    return model.bert_pretrained if hasattr(model, "bert_pretrained") else model


def frozen_reference(model):
    """The thing to pass as `lm_reference`: a deep copy of `model` as it is now, in eval mode, with requires_grad_(False) on
    every parameter.  (The copy's engine starts empty and builds its own weight copies at its first forward.)"""
    ref = copy.deepcopy(model)
    ref.eval()
    ref.requires_grad_(False)
    for p in ref.parameters():
        p.grad = None
    return ref


_REF_CONFIG_KEYS = ("vocab_size", "hidden_size", "v_hidden_size", "bi_hidden_size", "num_hidden_layers", "v_num_hidden_layers",
                    "num_attention_heads", "v_num_attention_heads", "bi_num_attention_heads", "intermediate_size",
                    "v_intermediate_size", "bi_intermediate_size", "v_feature_size", "v_target_size", "v_biattention_id",
                    "t_biattention_id", "with_coattention", "fixed_t_layer", "fixed_v_layer", "max_position_embeddings",
                    "type_vocab_size")


def check_reference(model, lm_reference, obj):
    """The refused uses of `lm_reference` (ValueError, before anything touches the device) -> the reference's pre-training
    model when the step's objective reads it (kl_coef > 0, or a PreferenceObjective), else None.  model: the trained
    BertForMultiModalPreTraining."""
    pref = isinstance(obj, PreferenceObjective)
    if lm_reference is None:
        if obj is not None and not pref and obj.kl_coef > 0:
            raise ValueError(f"PolicyObjective(kl_coef={obj.kl_coef}) penalises KL(p || p_ref): pass lm_reference "
                             "(policy.frozen_reference(model), taken before the fine-tune), or kl_coef=0")
        return None
    if obj is None:
        raise ValueError("lm_reference is the frozen model of the policy-gradient objective's KL term: pass lm_advantage (and "
                         "PolicyObjective(kl_coef=...)) with it, or drop it for the likelihood objective")
    ref = _pretraining_model(lm_reference)
    if ref is model:
        raise ValueError("lm_reference is the trained model itself: its KL to itself is 0 and it would move with every step; "
                         "pass a frozen copy, policy.frozen_reference(model)")
    if not (hasattr(ref, "config") and hasattr(ref, "_engine") and hasattr(ref, "compute_dtype")):
        raise ValueError(f"lm_reference must be a BertForMultiModalPreTraining or a VisualDialogEncoder, got {type(lm_reference).__name__}")
    diff = [k for k in _REF_CONFIG_KEYS if getattr(ref.config, k, None) != getattr(model.config, k, None)]
    if diff:
        raise ValueError("lm_reference must have the trained model's vocabulary, hidden sizes and layer schedule; its config "
                         f"differs in {', '.join(diff)}")
    if ref.compute_dtype != "bf16":
        raise ValueError(f"lm_reference must run on the bf16 engine (compute_dtype='bf16'), got {ref.compute_dtype!r}")
    if ref._device() != model._device():
        raise ValueError(f"lm_reference is on {ref._device()}, the trained model on {model._device()}: move it with .to()")
    return ref if (pref or obj.kl_coef > 0) else None


_TEACHER_CONFIG_KEYS = ("vocab_size", "v_feature_size", "type_vocab_size", "max_position_embeddings")


def check_teacher(model, lm_reference):
    """The refused teachers of a `DistillObjective` (ValueError, before anything touches the device) -> the teacher's pre-training
    model.  Unlike `check_reference` it asks only for what the shared inputs and the logits row depend on: the vocabulary, the
    region feature size, the segment vocabulary and the position table; depth, widths, head counts, intermediate sizes, the
    connection schedule and the frozen layers are the teacher's own.  model: the trained BertForMultiModalPreTraining."""
    ref = _pretraining_model(lm_reference)
    if ref is model:
        raise ValueError("lm_reference is the trained model itself: the distillation term against itself is 0 and it would move "
                         "with every step; pass a separate teacher, or policy.frozen_reference(model) for self-distillation")
    if not (hasattr(ref, "config") and hasattr(ref, "_engine") and hasattr(ref, "compute_dtype")):
        raise ValueError(f"the teacher (lm_reference) must be a BertForMultiModalPreTraining or a VisualDialogEncoder, got "
                         f"{type(lm_reference).__name__}")
    diff = [k for k in _TEACHER_CONFIG_KEYS if getattr(ref.config, k, None) != getattr(model.config, k, None)]
    if diff:
        raise ValueError("the teacher (lm_reference) must read the student's inputs and predict over its vocabulary; its config "
                         f"differs in {', '.join(diff)}")
    if ref.compute_dtype != "bf16":
        raise ValueError(f"the teacher (lm_reference) must run on the bf16 engine (compute_dtype='bf16'), got {ref.compute_dtype!r}")
    if ref._device() != model._device():
        raise ValueError(f"the teacher (lm_reference) is on {ref._device()}, the trained model on {model._device()}: move it with .to()")
    return ref


def check_distill_inputs(lm_objective, lm_reference, lm_advantage, lm_behaviour_logp, lm_preference, compute_dtype, train_branch=True):
    """The refused combinations of the distillation arguments of `forward` / `forward_backward` (ValueError, before anything
    touches the device) -> the objective in force.  `lm_weight` is allowed: it weighs the hard-label term as it weighs the
    likelihood.  lm_reference: only its presence is judged here (`check_teacher` judges the model)."""
    for name, t in (("lm_advantage", lm_advantage), ("lm_behaviour_logp", lm_behaviour_logp), ("lm_preference", lm_preference)):
        if t is not None:
            raise ValueError(f"lm_objective=DistillObjective (knowledge distillation) and {name} describe two objectives for the "
                             "same rows: pass one of them")
    _check_distill_values(lm_objective.temperature, lm_objective.alpha)
    if lm_reference is None:
        raise ValueError("DistillObjective fits the student to a teacher's distribution: pass the teacher as lm_reference (a "
                         "frozen model of either class; policy.frozen_reference(model) for self-distillation)")
    if compute_dtype != "bf16":
        raise ValueError(f"the distillation objective runs on the bf16 engine only: build the model with compute_dtype='bf16' "
                         f"(got {compute_dtype!r})")
    if not train_branch:
        raise ValueError("DistillObjective replaces the LM loss of the train branch: pass masked_lm_labels, next_sentence_label and "
                         "image_target with it (this call computes no loss and would ignore it)")
    return lm_objective


def check_policy_inputs(shape, lm_advantage, lm_behaviour_logp, lm_objective, lm_weight, compute_dtype, train_branch=True,
                        lm_reference=None):
    """The refused combinations of the policy-gradient arguments of `forward` / `forward_backward` (ValueError, before
    anything touches the device) -> the objective in force (None without `lm_advantage`).  train_branch: whether the call
    computes the losses (labels, NSP label and image target all given).  lm_reference: only its presence is judged here
    (`check_reference` judges the model)."""
    if lm_advantage is None:
        if lm_reference is not None:
            check_reference(None, lm_reference, None)
        if lm_behaviour_logp is not None or lm_objective is not None:
            raise ValueError("lm_behaviour_logp / lm_objective describe the policy-gradient objective: pass lm_advantage "
                             "(fp32 [B, T]) with them, or drop them for the likelihood objective")
        return None
    if lm_weight is not None:
        raise ValueError("lm_weight (the integer likelihood / unlikelihood weights) and lm_advantage (the policy-gradient "
                         "objective) are two objectives for the same rows: pass one of them")
    if compute_dtype != "bf16":
        raise ValueError(f"the policy-gradient objective runs on the bf16 engine only: build the model with "
                         f"compute_dtype='bf16' (got {compute_dtype!r})")
    obj = PolicyObjective() if lm_objective is None else lm_objective
    if not isinstance(obj, PolicyObjective):
        raise ValueError(f"lm_objective must be a policy.PolicyObjective, got {type(lm_objective).__name__}")
    if obj.mode == "ratio" and lm_behaviour_logp is None:
        raise ValueError("PolicyObjective(mode='ratio') weighs each token by p / q: pass lm_behaviour_logp (fp32 [B, T], the "
                         "step_logq of generate_answers spread over the copy rows), or use mode='logp'")
    B, T = (int(x) for x in shape)
    for name, t in (("lm_advantage", lm_advantage), ("lm_behaviour_logp", lm_behaviour_logp)):
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != (B, T)):
            got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"{name} must be a tensor of shape [B, T] = {(B, T)} like input_ids (one value per token, read on "
                             f"the labelled rows), got {got}: build it with policy.spread")
    if obj.kl_coef > 0 and lm_reference is None:
        check_reference(None, None, obj)
    if not train_branch:
        raise ValueError("lm_advantage weighs the LM loss of the train branch: pass masked_lm_labels, next_sentence_label and "
                         "image_target with it (this call computes no loss and would ignore it)")
    return obj


def bind_objective(model, shape, train_branch=True, *, lm_advantage=None, lm_behaviour_logp=None, lm_objective=None,
                   lm_reference=None, lm_preference=None, lm_weight=None):
    """The objective keywords of `forward` / `forward_backward` (input_ids of `shape`), judged once by the checks above -> all
    the engine sees of them: the step's bound objective (unimm_amd/lm_objective.py), None for the likelihood step.  model: the trained one."""
    if isinstance(lm_objective, DistillObjective):
        obj = check_distill_inputs(lm_objective, lm_reference, lm_advantage, lm_behaviour_logp, lm_preference, model.compute_dtype,
                                   train_branch)
        return LO.Distillation(obj, check_teacher(model, lm_reference))
    if lm_preference is not None:
        obj = check_preference_inputs(shape, lm_preference, lm_objective, lm_advantage, lm_weight, lm_behaviour_logp,
                                      model.compute_dtype, train_branch)
    else:
        obj = check_policy_inputs(shape, lm_advantage, lm_behaviour_logp, lm_objective, lm_weight, model.compute_dtype, train_branch,
                                  lm_reference=lm_reference)
    reference = check_reference(model, lm_reference, obj)
    if lm_preference is not None:
        return LO.Preference(lm_preference, obj, shape[1], reference)
    return None if obj is None else LO.PolicyGradient(lm_advantage, lm_behaviour_logp, obj, reference)


@dataclass
class SampledBatch:
    """The sampled answers of G dialogs as K <= G * N generative training sequences of T tokens (hypotheses of length 0 dropped)."""
    input_ids: torch.Tensor          # int64 [K, T]: context, answer tokens + [SEP], the [MASK] copy block
    token_type_ids: torch.Tensor     # int64 [K, T]
    position_ids: torch.Tensor       # int64 [K, T]
    masked_lm_labels: torch.Tensor   # int64 [K, T]: -1 except on the copy rows (the answer's tokens + [SEP])
    attention_mask: DialogMaskSpec   # mode 1, length c + n, answer n
    image_index: torch.Tensor        # int64 [K]: the sequence's dialog (= its image)
    copy_rows: torch.Tensor          # bool [K, T]
    kept: torch.Tensor               # int64 [K]: g * N + j of every sequence
    shape: tuple                     # (G, N)


def sampled_training_batch(input_ids, token_type_ids, position_ids, context_len, answers, T):
    """G dialog contexts (the first context_len[g] tokens of input_ids / token_type_ids / position_ids, as `generate_answers`
    took them) + a GeneratedAnswers with N hypotheses each -> SampledBatch.  Answer token k and its [MASK] copy get position id
    position_ids[g, c-1] + 1 + k and segment token_type_ids[g, c-1] ^ 1 (generation.answer_ids)."""
    ids, tt, pp = (np.asarray(t.cpu() if torch.is_tensor(t) else t).astype(np.int64) for t in (input_ids, token_type_ids, position_ids))
    c_all = np.asarray(context_len.cpu() if torch.is_tensor(context_len) else context_len).astype(np.int64).reshape(-1)
    tokens = answers.tokens.cpu().numpy().astype(np.int64)
    lengths = answers.lengths.cpu().numpy().astype(np.int64)
    G, N = lengths.shape
    if ids.shape[0] != G or c_all.shape[0] != G:
        raise ValueError(f"sampled_training_batch: {ids.shape[0]} contexts / {c_all.shape[0]} context lengths for the answers of {G} dialogs")
    kept = [(g, j) for g in range(G) for j in range(N) if lengths[g, j] > 0]
    K = len(kept)
    out_ids, out_tt, out_pp = (np.zeros((K, T), np.int64) for _ in range(3))
    labels = np.full((K, T), -1, np.int64)
    copy = np.zeros((K, T), bool)
    L, n_all = np.zeros(K, np.int64), np.zeros(K, np.int64)
    for k, (g, j) in enumerate(kept):
        c, n = int(c_all[g]), int(lengths[g, j])
        if c + 2 * n > T:
            raise ValueError(f"sampled_training_batch: dialog {g} (context {c}) with an answer of {n} tokens needs {c + 2 * n} "
                             f"positions, more than T = {T}: generate with the same T")
        ans = tokens[g, j, :n]
        out_ids[k, :c], out_tt[k, :c], out_pp[k, :c] = ids[g, :c], tt[g, :c], pp[g, :c]
        out_ids[k, c:c + n], out_ids[k, c + n:c + 2 * n] = ans, MASK
        out_tt[k, c:c + 2 * n] = tt[g, c - 1] ^ 1
        out_pp[k, c:c + n] = out_pp[k, c + n:c + 2 * n] = pp[g, c - 1] + 1 + np.arange(n)
        labels[k, c + n:c + 2 * n] = ans
        copy[k, c + n:c + 2 * n] = True
        L[k], n_all[k] = c + n, n
    T_ = torch.from_numpy
    flat = np.array([g * N + j for g, j in kept], np.int64)
    return SampledBatch(input_ids=T_(out_ids), token_type_ids=T_(out_tt), position_ids=T_(out_pp), masked_lm_labels=T_(labels),
                        attention_mask=DialogMaskSpec(np.ones(K), L, n_all), image_index=T_(flat // max(N, 1)),
                        copy_rows=T_(copy), kept=T_(flat), shape=(G, N))


def candidate_training_batch(input_ids, token_type_ids, position_ids, context_len, answer_tokens, answer_lengths, T):
    """`sampled_training_batch` for GIVEN candidates: answer_tokens [G, N, W] holds each candidate's tokens, then [SEP], zero-padded;
    answer_lengths [G, N] counts the tokens and the [SEP], 0 = the candidate is absent (dropped, as a length-0 sample is) ->
    the same SampledBatch.  Targets [G, N] reach the step's sequences as `PreferenceTargets(batch.image_index,
    targets.reshape(-1)[batch.kept])`."""
    from .generation import GeneratedAnswers
    tok = torch.as_tensor(answer_tokens).detach().to("cpu", torch.int64)
    length = torch.as_tensor(answer_lengths).detach().to("cpu", torch.int64)
    if tok.dim() != 3 or tuple(length.shape) != tuple(tok.shape[:2]):
        raise ValueError(f"candidate_training_batch: answer_tokens must be [G, N, W] and answer_lengths [G, N], got "
                         f"{tuple(tok.shape)} / {tuple(length.shape)}")
    if length.numel() and (int(length.min()) < 0 or int(length.max()) > tok.shape[2]):
        raise ValueError(f"candidate_training_batch: answer_lengths must lie in [0, W = {tok.shape[2]}]")
    zeros = torch.zeros(tuple(length.shape), dtype=torch.float32)
    return sampled_training_batch(input_ids, token_type_ids, position_ids, context_len,
                                  GeneratedAnswers(tokens=tok, lengths=length, scores=zeros, logp=zeros,
                                                   step_logp=torch.zeros(tuple(tok.shape), dtype=torch.float32)), T)


def spread(values, batch: SampledBatch):
    """values [G, N] (one per sequence) or [G, N, W] (one per answer token: step_logq / step_logp) -> fp32 [K, T] with the
    value(s) on the sequence's copy rows and zero elsewhere."""
    v = torch.as_tensor(values).detach().to("cpu", torch.float32)
    G, N = batch.shape
    if tuple(v.shape[:2]) != (G, N) or v.dim() not in (2, 3):
        raise ValueError(f"spread: values must be [G, N] or [G, N, W] with (G, N) = {(G, N)}, got {tuple(v.shape)}")
    per_sequence = v.dim() == 2
    v = v.reshape(G * N, -1)[batch.kept]                       # [K, 1 | W]
    n = batch.copy_rows.sum(1)
    out = torch.zeros(batch.copy_rows.shape, dtype=torch.float32)
    if per_sequence:
        out[batch.copy_rows] = v[:, 0].repeat_interleave(n)
    else:
        if int(n.max()) > v.shape[1]:
            raise ValueError(f"spread: {v.shape[1]} values per answer, but an answer has {int(n.max())} tokens")
        out[batch.copy_rows] = v[torch.arange(v.shape[1])[None, :] < n[:, None]]
    return out


def self_critical_advantage(rewards, baseline):
    """rewards [G, N] -> advantages [G, N] (fp32, host).  baseline: a [G] tensor (the reward of the dialog's greedy answer:
    self-critical sequence training), "mean" (for sample j the mean reward of the dialog's OTHER samples; N >= 2) or None."""
    r = torch.as_tensor(rewards).detach().to("cpu", torch.float32)
    if r.dim() != 2:
        raise ValueError(f"self_critical_advantage: rewards must be [G, N], got {tuple(r.shape)}")
    if baseline is None:
        return r.clone()
    if isinstance(baseline, str):
        if baseline != "mean":
            raise ValueError(f"self_critical_advantage: baseline must be a [G] tensor, 'mean' or None, got {baseline!r}")
        N = r.shape[1]
        if N < 2:
            raise ValueError("self_critical_advantage: baseline='mean' is the mean of the other samples and needs N >= 2")
        return r - (r.sum(1, keepdim=True) - r) / (N - 1)
    b = torch.as_tensor(baseline).detach().to("cpu", torch.float32).reshape(-1)
    if b.shape[0] != r.shape[0]:
        raise ValueError(f"self_critical_advantage: {b.shape[0]} baselines for {r.shape[0]} dialogs")
    return r - b[:, None]
