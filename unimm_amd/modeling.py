"""Drop-in model surface: `BertForMultiModalPreTraining(config)` and `VisualDialogEncoder(config_path)`
with the reference's constructor / forward() signatures, return tuples and `state_dict` names
(models/vilbert_dialog.py:1496-1626, models/visual_dialog_encoder.py:8-50), computed by the HIP
engine (unimm_amd.engine).  The modules below only own parameters; all arithmetic is in the kernels.
"""
from __future__ import annotations

import logging
import os
import warnings

import torch
from torch import nn

from . import params as PM
from .config import BertConfig
from .engine import Engine
from .lm_objective import KEY as OBJECTIVE_KEY
from .policy import bind_objective

logger = logging.getLogger(__name__)

# the arguments of `forward` / `forward_backward` that reach the engine as they are; the shared-context pass
# (unimm_amd/scoring.py) reads, and gets staged, the first ten only
_SHARED_INPUTS = ("input_ids", "image_feat", "image_loc", "token_type_ids", "position_ids", "attention_mask", "image_attention_mask",
                  "masked_lm_labels", "lm_weight", "image_index")
_INPUTS = _SHARED_INPUTS + ("co_attention_mask", "image_label", "image_target", "next_sentence_label", "nsp_weight")
_OBJECTIVE_ARGS = ("lm_advantage", "lm_behaviour_logp", "lm_objective", "lm_reference", "lm_preference", "lm_weight")


def _build_param_tree(root: nn.Module, cfg) -> None:
    """Register every parameter under nested plain containers so that state_dict keys equal the
    reference's ("bert.encoder.layer.0.attention.self.query.weight", ...).  Init follows
    init_bert_weights (models/vilbert_dialog.py:1110-1121): N(0, initializer_range) for Linear /
    Embedding weights, zero biases, LayerNorm weight 1 / bias 0."""
    for name, shape in PM.state_dict_names(cfg).items():
        if name == PM.TIED_DECODER:
            continue
        parts = name.split(".")
        mod = root
        for part in parts[:-1]:
            if not hasattr(mod, part):
                mod.add_module(part, nn.Module())
            mod = getattr(mod, part)
        if "LayerNorm" in name:
            t = torch.ones(shape) if parts[-1] == "weight" else torch.zeros(shape)
        elif parts[-1] == "weight":
            t = torch.empty(shape).normal_(mean=0.0, std=cfg.initializer_range)
        else:
            t = torch.zeros(shape)
        mod.register_parameter(parts[-1], nn.Parameter(t))
    # tie the decoder to the word embeddings (models/vilbert_dialog.py:1020, :1504-1506)
    root.cls.predictions.add_module("decoder", nn.Module())
    root.cls.predictions.decoder.register_parameter("weight", root.bert.embeddings.word_embeddings.weight)


def load_pretrained_state_dict(model: nn.Module, state_dict, default_gpu=True):
    """models/vilbert_dialog.py:1232-1296 on a plain key -> tensor mapping.  Returns (missing_keys, unexpected_keys)."""
    sd = {}
    for key, v in state_dict.items():
        new_key = key
        if "gamma" in new_key:
            new_key = new_key.replace("gamma", "weight")
        if "beta" in new_key:
            new_key = new_key.replace("beta", "bias")
        if new_key.startswith("bert_pretrained."):          # a VisualDialogEncoder checkpoint (train.py:503-505)
            new_key = new_key[len("bert_pretrained."):]
        sd[new_key] = v
    start_prefix = ""
    if not hasattr(model, "bert") and any(k.startswith("bert.") for k in sd):
        start_prefix = "bert."
    own = model.state_dict()
    missing, errors, usable = [], [], {}
    for k, t in own.items():
        src = sd.get(start_prefix + k)
        if src is None:
            missing.append(k)
        elif tuple(src.shape) != tuple(t.shape):
            errors.append(f"size mismatch for {k}: copying a param with shape {tuple(src.shape)} from checkpoint, "
                          f"the shape in current model is {tuple(t.shape)}.")
        else:
            usable[k] = src
    expected = {start_prefix + k for k in own}
    unexpected = [k for k in sd if k not in expected]
    if errors and default_gpu:
        raise RuntimeError("Error(s) in loading state_dict for {}:\n\t{}".format(model.__class__.__name__, "\n\t".join(errors)))
    model.load_state_dict(usable, strict=False)
    if missing and default_gpu:
        logger.info("Weights of {} not initialized from pretrained model: {}".format(model.__class__.__name__, missing))
    if unexpected and default_gpu:
        logger.info("Weights from pretrained model not used in {}: {}".format(model.__class__.__name__, unexpected))
    return missing, unexpected


class _HotPath(torch.autograd.Function):
    """One autograd node for the whole forward/backward hot path.  Parameter gradients are
    accumulated in place into the flat gradient arena (every Parameter's .grad is a view of it), so
    backward returns no tensors; `anchor` only makes autograd call us."""

    @staticmethod
    def forward(ctx, anchor, engine, inp, opts):
        ctx.set_materialize_grads(False)
        ctx.graph_entry = None
        if engine.graphs is not None and engine.graphs.eligible(inp, opts):     # the step as two replayed hipGraphs
            res = engine.graphs.forward(inp, opts)
            if res is not None:
                ctx.engine, ctx.out, ctx.graph_entry = engine, None, res[4]
                ctx.graph_token = res[4].out.pop("_token", None)   # alive until backward ran: the entry is not replayed meanwhile
                engine.last_seq_t = (None, None)
                return res[0], res[1], res[2], res[3]
        out = engine.forward(inp, train=opts["train"], save=True, lm_rows="labelled", want_pred_v=True,
                             want_seq=bool(opts["want_seq"]))
        losses = engine.losses(out, inp)
        ctx.engine, ctx.out = engine, out
        engine.last_seq_t = (engine.padded(out, out["seq32_t"]) if opts["want_seq"] else None,
                             engine.padded(out, out["seq_out_t"]) if opts["want_seq"] else None)
        nsp = out["nsp"].clone()
        return losses["lm_loss"], losses["img_loss"], losses["nsp_loss"], nsp

    @staticmethod
    def backward(ctx, g_lm, g_img, g_nsp, g_scores):
        engine, out = ctx.engine, ctx.out
        ctx.out = None
        if ctx.graph_entry is not None:
            engine.graphs.backward(ctx.graph_entry, g_lm, g_img, g_nsp, g_scores)
            ctx.graph_token = None
            return None, None, None, None
        engine.backward(out, g_lm, g_img, g_nsp, g_scores)
        return None, None, None, None


class BertForMultiModalPreTraining(nn.Module):
    """BERT model with multi modal pre-training heads (drop-in for models/vilbert_dialog.py:1496)."""

    def __init__(self, config, compute_dtype="bf16"):
        """`compute_dtype` (an extension of the reference's one-argument constructor): "bf16" = the reference's autocast
        class (train.py:445: half-precision matmuls, fp32 LayerNorm / softmax / losses) on the bf16 MFMA engine; "fp32x3" =
        fp32-grade arithmetic end to end for callers that run WITHOUT autocast (dense_annotation_finetuning.py:253), on the
        same GEMM kernels over split operands (unimm_amd/engine_x3.py)."""
        super().__init__()
        if not isinstance(config, BertConfig):
            raise ValueError(
                "Parameter config in `{}(config)` should be an instance of class `BertConfig`. ".format(
                    self.__class__.__name__))
        self.config = config
        _build_param_tree(self, config)
        self.predict_feature = config.predict_feature
        if compute_dtype not in ("bf16", "fp32x3"):
            raise ValueError(f"compute_dtype must be 'bf16' or 'fp32x3', got {compute_dtype!r}")
        self.compute_dtype = compute_dtype
        if compute_dtype == "fp32x3":
            from .engine_x3 import EngineX3
            self._engine = EngineX3(self, config)
        else:
            self._engine = Engine(self, config)
        # values loaded into the Parameters must reach the engine's bf16 / transposed weight copies
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._engine.invalidate_weights())

    # -- construction helpers -----------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, config, default_gpu=True, state_dict=None, *inputs, **kwargs):
        """Key handling of models/vilbert_dialog.py:1232-1296.  The reference downloads 'bert-base-uncased' here
        (:1123-1231); there is no network in this build, so weights come from `state_dict` or from a local
        checkpoint file / directory at the given path, otherwise the model keeps its fresh init (with a warning).
        A found state dict is loaded as the reference loads it: old LayerNorm names (`gamma` / `beta`) are renamed to
        `weight` / `bias` (:1233-1245), the `bert.` start prefix is detected (:1270-1274), every key of the model that
        the checkpoint lacks is reported as missing and every checkpoint key the model lacks as unexpected
        (:1276-1287, logged when `default_gpu`), and a shape mismatch raises (:1288-1294)."""
        model = cls(config, *inputs, **kwargs)
        if state_dict is None and isinstance(pretrained_model_name_or_path, str):
            path = pretrained_model_name_or_path
            if os.path.isdir(path):
                path = os.path.join(path, "pytorch_model.bin")
            if os.path.isfile(path):
                state_dict = torch.load(path, map_location="cpu")
        if state_dict is None:
            warnings.warn(f"from_pretrained({pretrained_model_name_or_path!r}): no local weights found, "
                          "keeping random initialisation (no network access)")
            return model
        missing, unexpected = load_pretrained_state_dict(model, state_dict, default_gpu=default_gpu)
        model.pretrained_missing_keys, model.pretrained_unexpected_keys = missing, unexpected
        return model

    @property
    def engine(self) -> Engine:
        return self._engine

    def set_dropout_seed(self, seed: int, step: int = 0):
        self._engine.seed, self._engine.step = int(seed), int(step)

    # -- forward ---------------------------------------------------------------------------------
    def forward(self, input_ids, image_feat, image_loc, sep_indices=None, sep_len=None, token_type_ids=None,
                position_ids=None, attention_mask=None, image_attention_mask=None, co_attention_mask=None,
                masked_lm_labels=None, image_label=None, image_target=None, next_sentence_label=None,
                output_all_attention_masks=False, nsp_weight=None, lm_weight=None,
                _want_lm_scores=True, _want_pred_v=True, image_index=None, lm_advantage=None, lm_behaviour_logp=None,
                lm_objective=None, lm_reference=None, lm_preference=None, shared_context=None):
        """Same contract as models/vilbert_dialog.py:1519-1626.  `sep_indices` / `sep_len` are accepted and
        ignored exactly as the reference's embeddings do (:326-356).  Train branch (labels, NSP label and
        image target all given) -> (lm_loss[1], img_loss[1], nsp_loss[1], seq_out_t, pred_t, nsp[B,2]);
        otherwise -> (pred_t, pred_v, nsp, seq_out_t, attention-lists).
        `_want_lm_scores=False` (used by VisualDialogEncoder when the caller does not ask for LM scores)
        skips materialising the dense [B,T,vocab] logits; the loss only ever needs the labelled rows.
        Extensions (unimm_amd/inputs.py): `attention_mask` may be a `DialogMaskSpec`
        (then `co_attention_mask` must be None) and `image_feat` / `image_loc` / `image_target` may hold one
        entry per IMAGE with `image_index` [B] mapping sequences to them.  `lm_advantage` (fp32 [B, T], with
        `lm_behaviour_logp` and `lm_objective`: unimm_amd/policy.py) makes lm_loss the policy-gradient objective on the
        labelled rows instead of the weighted likelihood; bf16 engine, train branch.  `lm_reference` (a frozen model of either
        class, `policy.frozen_reference`) is what `PolicyObjective(kl_coef > 0)` measures KL(p || p_ref) against: its engine runs
        an inference forward on this call's inputs first; with kl_coef == 0 it is ignored.  `lm_preference`
        (`policy.PreferenceTargets`: a group id and a target weight per sequence, with `lm_objective=policy.PreferenceObjective`
        and optionally `lm_reference`) makes lm_loss the listwise preference objective over the candidate answers of each group
        instead; bf16 engine, train branch; the step's per-sequence results are in `engine.last_lm_preference`.
        `lm_objective=policy.DistillObjective(temperature, alpha)` with `lm_reference=teacher` (a frozen model of either class, of
        any depth and width over the same vocabulary and inputs) makes lm_loss the token-level distillation objective on the
        labelled rows, `lm_weight` still weighing its hard-label share; bf16 engine, train branch; `engine.last_lm_distill`.  With
        `shared_context` (and `lm_preference`; the conditions of `forward_backward(shared_context=)`) that loss is computed on the
        shared-context schedule, as a value only -- no autograd graph: train with `forward_backward` -- and the call returns
        (lm_loss, 0, 0, None, None, None)."""
        args = locals()                        # the call's arguments by name (`_bind_objective`, `_engine_inputs`)
        train_branch = masked_lm_labels is not None and next_sentence_label is not None and image_target is not None
        if shared_context is not None:
            if lm_preference is None:
                raise ValueError("forward(shared_context=...) evaluates the preference loss on the shared schedule: pass "
                                 "lm_preference with it (sequence_log_likelihood and forward_backward take shared_context otherwise)")
            if masked_lm_labels is None:
                raise ValueError("forward(shared_context=...) needs masked_lm_labels (the copy rows)")
            train_branch = True
        objective = self._bind_objective(args, (1.0, 0.0, 0.0), train_branch)
        eng = self._engine
        inp = self._engine_inputs(objective, shared_context is not None, args)
        if shared_context is not None:
            _, lm_loss, zero = self._shared_step(inp, shared_context, None)
            return lm_loss, zero, zero.clone(), None, None, None
        B, T = input_ids.shape
        H, V = self.config.hidden_size, self.config.vocab_size
        if train_branch:
            if torch.is_grad_enabled():
                lm_loss, img_loss, nsp_loss, nsp = _HotPath.apply(eng._anchor, eng, inp,
                                                                  dict(train=self.training, want_seq=_want_lm_scores))
                seq_raw = eng.last_seq_t
            else:
                out = eng.forward(inp, train=self.training, save=False, lm_rows="labelled", want_pred_v=True)
                ls = eng.losses(out, inp)
                lm_loss, img_loss, nsp_loss, nsp = ls["lm_loss"], ls["img_loss"], ls["nsp_loss"], out["nsp"]
                seq_raw = (eng.padded(out, out["seq32_t"]), eng.padded(out, out["seq_out_t"])) if _want_lm_scores else None
            eng.last_seq_t = None
            seq_t = pred_t = None
            if _want_lm_scores:
                with torch.no_grad():   # dense scores are an output only; the loss path is row-sparse
                    seq_t = seq_raw[0].view(B, T, H)
                    pred_t = eng.decode_rows(seq_raw[1], B * T).view(B, T, -1)[:, :, :V]
            return lm_loss, img_loss, nsp_loss, seq_t, pred_t, nsp
        att = ([], [], [])
        with torch.no_grad():
            if output_all_attention_masks:     # :855-929, :1626 -- diagnostic output, padded one-stream schedule
                out, att = eng.forward_with_attention(inp, train=self.training, lm_rows="all" if _want_lm_scores else "none",
                                                      want_pred_v=_want_pred_v)
            else:
                out = eng.forward(inp, train=self.training, save=False, lm_rows="all" if _want_lm_scores else "none",
                                  want_pred_v=_want_pred_v)
        seq_t = eng.padded(out, out["seq32_t"]).view(B, T, H)
        return out.get("pred_t"), out.get("pred_v"), out["nsp"], seq_t, att

    def forward_backward(self, input_ids, image_feat, image_loc, loss_weights, sep_indices=None, sep_len=None, token_type_ids=None,
                         position_ids=None, attention_mask=None, image_attention_mask=None, co_attention_mask=None,
                         masked_lm_labels=None, image_label=None, image_target=None, next_sentence_label=None, nsp_weight=None,
                         lm_weight=None, image_index=None, plan_header=None, lm_advantage=None, lm_behaviour_logp=None,
                         lm_objective=None, shared_context=None, lm_reference=None, lm_preference=None):
        """The training step's forward AND backward in one call (an extension; the reference writes
        `loss = c_lm * lm.mean() + c_nsp * nsp.mean() + c_img * img.mean(); loss.backward()`, train.py:164-168, :315).
        loss_weights = (c_lm, c_nsp, c_img).  With the weights known up front the backward does not wait for the host to see
        the losses: both halves are enqueued back to back (two graph replays under the step executor) -- no autograd round trip
        (a hand-over to the autograd thread and ~8 one-element launches between the halves: 0.2-0.4 ms during which a
        30-sequence step's GPU idles).  Parameter gradients accumulate into `.grad` exactly as with `loss.backward()`.
        -> (loss, lm_loss, img_loss, nsp_loss, nsp_logits).  plan_header: `engine.count_rows(...)` of this batch if the caller
        has it already (a prefetcher: the step then starts without its host sync).  lm_advantage / lm_behaviour_logp /
        lm_objective / lm_reference: as in `forward` (the policy-gradient step always runs eagerly; with a shared context the
        reference runs the shared pass as well).
        shared_context (an extension): one group id per sequence, as in `sequence_log_likelihood` -- the sequences of a group
        share image and dialog context and differ only in the answer (the N sampled answers of a dialog, unimm_amd/policy.py).
        A bare list admits answers of up to 14 tokens (32 private rows); `SharedContext(ids, 64)` admits up to 30 (ValueError beyond).
        The context rows and the image stream then run ONCE per group, forward and backward (unimm_amd/scoring.py); only the LM
        term is trained: loss_weights must be (c, 0, 0), attention_mask a generative-mode DialogMaskSpec, the engine bf16 with
        its connection layers and no frozen layers (ValueError otherwise).  The image and NSP losses come back as zeros and
        nsp_logits as None; when a sequence's context does not match its group's, the loss is NaN and the call adds nothing to
        the gradients.  Always eager.
        lm_preference / lm_objective=PreferenceObjective / lm_reference: as in `forward`, on either schedule (always eager)."""
        args = locals()                        # the call's arguments by name (`_bind_objective`, `_engine_inputs`)
        objective = self._bind_objective(args, loss_weights, True)
        if shared_context is not None:
            if masked_lm_labels is None:
                raise ValueError("forward_backward(shared_context=...) needs masked_lm_labels (the copy rows)")
        elif masked_lm_labels is None or next_sentence_label is None or image_target is None:
            raise ValueError("forward_backward needs the training inputs (masked_lm_labels, next_sentence_label, image_target)")
        eng, dev = self._engine, self._device()
        inp = self._engine_inputs(objective, shared_context is not None, args)
        if shared_context is not None:
            g_lm, lm_loss, zero = self._shared_step(inp, shared_context, loss_weights[0])
            return (g_lm * lm_loss).reshape(()), lm_loss, zero, zero.clone(), None
        if plan_header is not None:
            inp["_plan_header"] = plan_header
        c_lm, c_nsp, c_img = (float(c) for c in loss_weights)
        key = (c_lm, c_nsp, c_img, dev)
        seeds = self._fb_seeds.get(key) if hasattr(self, "_fb_seeds") else None
        if seeds is None:
            if not hasattr(self, "_fb_seeds"):
                self._fb_seeds = {}
            w = torch.tensor([c_lm, c_img, c_nsp], dtype=torch.float32, device=dev)
            seeds = self._fb_seeds[key] = (w[0:1], w[1:2], w[2:3], w)
        g_lm, g_img, g_nsp, w = seeds
        opts = dict(train=self.training, want_seq=False)
        with torch.no_grad():
            res = None
            if eng.graphs is not None and eng.graphs.eligible(inp, opts):
                res = eng.graphs.forward(inp, opts, defer_outputs=True)
            if res is not None:
                ent = res[4]
                tok = ent.out.pop("_token", None)
                eng.graphs.backward(ent, g_lm, g_img, g_nsp, None)
                del tok
                lm_loss, img_loss, nsp_loss, nsp = eng.graphs.outputs(ent)
            else:
                inp.pop("_plan_header", None)
                out = eng.forward(inp, train=self.training, save=True, lm_rows="labelled", want_pred_v=True, want_seq=False)
                ls = eng.losses(out, inp)
                lm_loss, img_loss, nsp_loss, nsp = ls["lm_loss"], ls["img_loss"], ls["nsp_loss"], out["nsp"].clone()
                eng.backward(out, g_lm.reshape(lm_loss.shape), g_img.reshape(img_loss.shape), g_nsp.reshape(nsp_loss.shape), None)
            eng.last_seq_t = None
            loss = torch.cat((lm_loss.reshape(1), img_loss.reshape(1), nsp_loss.reshape(1))).dot(w).reshape(())
        return loss, lm_loss, img_loss, nsp_loss, nsp

    def _bind_objective(self, args, loss_weights, train_branch):
        """Every refusal of the objective keywords and of the shared schedule, all on the host -> the call's bound objective or None."""
        shape = args["input_ids"].shape
        objective = bind_objective(self, shape, train_branch, **{k: args[k] for k in _OBJECTIVE_ARGS})
        if args["shared_context"] is not None:
            from .scoring import check_shared_training
            check_shared_training(self.config, self.compute_dtype, loss_weights, args["attention_mask"], args["shared_context"],
                                  shape[1], args["image_feat"].shape[1])
        return objective

    def _engine_inputs(self, objective, shared, args):
        """The engine's `inp` of one call: its tensor arguments (on the shared schedule the ones that pass reads; the [B, R]
        image key mask then stays a tensor, the pass indexes it by group) and the bound objective under its one key, the host
        tensors staged (the reference's callers pass CPU tensors, train.py:113-161); counts the step."""
        eng = self._engine
        eng.ensure(self._device())
        inp = {k: args[k] for k in (_SHARED_INPUTS if shared else _INPUTS)}
        if objective is not None:
            inp[OBJECTIVE_KEY] = objective
        eng.stage_host_inputs(inp, pack=() if shared else None)
        if self.training:
            eng.step += 1
        return inp

    def _shared_step(self, inp, shared_context, c_lm):
        """The LM term on the shared-context schedule: forward, loss and (c_lm not None) the backward of c_lm * lm_loss; no
        autograd graph -> (the gradient seed | None, lm_loss, a zero for the losses that take no part)."""
        eng, dev = self._engine, self._device()
        with torch.no_grad():
            g_lm = None if c_lm is None else torch.full((1,), float(c_lm), dtype=torch.float32, device=dev)
            lm_loss = eng.forward_backward_shared(inp, shared_context, g_lm, self.training)
            eng.last_seq_t = None
            zero = torch.zeros(1, dtype=torch.float32, device=dev)
        return g_lm, lm_loss, zero

    def _device(self):
        return self.bert.embeddings.word_embeddings.weight.device

    # generative scoring without the [B,T,vocab] tensor (val_lm.py:121-136 / val_avg_lm.py:135)
    @torch.no_grad()
    def sequence_log_likelihood(self, input_ids, image_feat, image_loc, masked_lm_labels, average=False, shared_context=None, **kw):
        """-sum_t CE(pred_t, labels, ignore_index=-1) per sequence, computed on the labelled rows only by
        the fused decoder + log-softmax kernels.  Returns (scores[B] fp32, nsp[B,2]).
        shared_context (an extension): one group id per sequence -- sequences of a group share image and dialog context and
        differ only in the candidate answer, as the 100 options of a round in val_lm.py:52-121 do (pass the round index).  A bare
        list admits candidates of up to 14 tokens; `SharedContext(ids, 64)` (unimm_amd/scoring.py) up to 30 (ValueError beyond).  The
        context rows and the image stream are then computed once per group (unimm_amd/scoring.py); a sequence whose context does
        not match its group comes back as NaN.  Both engines; on fp32x3 the two schedules differ only by the summation order
        inside the attention kernels (one unit in the last place of the scores in tests/test_gpu_x3_scoring.py)."""
        if shared_context is not None:
            from .scoring import sequence_log_likelihood_shared
            return sequence_log_likelihood_shared(self, input_ids, image_feat, image_loc, masked_lm_labels, shared_context,
                                                  average=average, **kw)
        eng = self._engine
        eng.ensure(self._device())
        inp = dict(input_ids=input_ids, image_feat=image_feat, image_loc=image_loc, masked_lm_labels=masked_lm_labels,
                   lm_weight=None, **kw)
        eng.stage_host_inputs(inp)                 # val_lm.py hands CPU tensors over chunk by chunk (val_lm.py:86-121)
        out = eng.forward(inp, train=False, save=False, lm_rows="labelled", want_pred_v=False)
        input_ids = inp["input_ids"]
        B, T = input_ids.shape
        scores = torch.zeros(B, dtype=torch.float32, device=eng.arena.device)
        lm = out.get("lm")
        if lm is not None:
            from . import lib as L
            seg = (lm["pos_idx"] // T).to(torch.int32)
            L.segment_sum(lm["rownll"], seg, scores, lm["n"], -1.0)
            if average:
                cnt = torch.bincount(seg.long(), minlength=B).clamp_min(1)
                scores = scores / cnt
        return scores, out["nsp"]

    @torch.no_grad()
    def generate_answers(self, input_ids, image_feat, image_loc, context_len, token_type_ids=None, position_ids=None,
                         image_attention_mask=None, image_index=None, *, beams=1, max_answer_len=20, min_answer_len=1,
                         length_penalty=0.0, banned_tokens=(0, 101, 103), samples=0, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                         sample_streams=None, greedy=False, no_repeat_ngram_size=0, repetition_penalty=1.0, repeat_scope="answer",
                         ensemble=None, ensemble_weights=None, ensemble_mode="prob", plausibility=0.0, draft_accept="match",
                         draft=None, draft_len=4):
        """Beam-search answers for the dialogs whose first context_len[g] tokens are `[CLS] caption [SEP] ... q_r [SEP]`, with the
        context and image computed once and a per-layer key/value cache (an extension; unimm_amd/generation.py states the
        semantics).  -> GeneratedAnswers(tokens, lengths, scores, logp).  bf16 engine.
        samples = 1 .. 16 (with beams = 1) DRAWS that many answers per dialog instead: temperature > 0, top_k (0 = off) and top_p
        (nucleus, 1 = off) shape the distribution, (seed, sample_streams[g] -- default the dialog's index) fix the draws; the
        result carries step_logq next to step_logp and keeps the samples in draw order.  temperature / top_k / top_p also take
        one value per draw; greedy=True decodes the greedy answer in the same pass (one more slot per dialog, samples <= 15) and
        returns it in `.greedy`.
        no_repeat_ngram_size = n in [1, 8] bans every id that would complete an n-gram the hypothesis has already produced,
        repetition_penalty = r != 1 ranks and draws the ids it has produced by x > 0 ? x * (1 / r) : x * r (beams = 1 or samples;
        step_logq reports the distribution drawn from, step_logp stays the model's); repeat_scope="dialog" makes the dialog's
        context tokens a second source of both rules.  unimm_amd/generation.py states them.
        draft = a second model of either class (its own depth and widths; policy.frozen_reference(model) to self-draft) makes the
        call SPECULATIVE greedy decoding (beams = 1, no sampling, no history rules): the draft proposes draft_len in [1, 15] tokens
        per round, this model verifies them in one pass and keeps the prefix it would have produced itself plus one token of its
        own.  The answers are those of the plain beams = 1 call; `.speculation` counts rounds, drafted and accepted tokens
        (unimm_amd/speculative.py).  draft_accept="rejection" (with samples >= 1) makes it speculative SAMPLING instead: the draft
        draws its proposals, the model accepts each with probability min(1, P / Q) or draws from the normalised max(0, P - Q)
        (`unimm_lm_spec_verify`), so the answers are distributed exactly as the plain sampling call's and carry step_logp / step_logq
        (and `.greedy` when asked); `.speculation` then counts per (dialog, draw).
        ensemble = 1 to 4 partner models of either class (their own depth and widths, this model's vocabulary and inputs;
        policy.frozen_reference(model) for a second copy of the same weights) makes every step decode all members on the same
        tokens and select from the MIXTURE of their next-token distributions (`unimm_lm_mix`): ensemble_mode="prob" the arithmetic
        mixture sum_m w_m p_m (ensemble_weights >= 0 summing to 1, this model's first, default uniform), "logit" the log-linear
        one sum_m w_m x_m with finite weights of any sign -- (1 + b, -b) with plausibility = alpha in (0, 1) is contrastive
        decoding: ids with p(id) < alpha * max p under THIS model are cut.  Beams, sampling, greedy=True and the step rules work
        unchanged, the history rules without a cut; step_logp is the log-probability under the normalised mixture."""
        from .generation import generate_answers
        return generate_answers(self, input_ids, image_feat, image_loc, context_len, token_type_ids, position_ids,
                                image_attention_mask, image_index, beams=beams, max_answer_len=max_answer_len,
                                min_answer_len=min_answer_len, length_penalty=length_penalty, banned_tokens=banned_tokens,
                                samples=samples, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                sample_streams=sample_streams, greedy=greedy, no_repeat_ngram_size=no_repeat_ngram_size,
                                repetition_penalty=repetition_penalty, repeat_scope=repeat_scope,
                                draft_accept=draft_accept, draft=draft, draft_len=draft_len, ensemble=ensemble,
                                ensemble_weights=ensemble_weights, ensemble_mode=ensemble_mode, plausibility=plausibility)


class VisualDialogEncoder(nn.Module):
    """Drop-in for models/visual_dialog_encoder.py:8-50 (what train.py / val_lm.py instantiate)."""

    def __init__(self, config_path, pretrained="bert-base-uncased", compute_dtype="bf16"):
        super().__init__()
        config = BertConfig.from_json_file(config_path)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.bert_pretrained = BertForMultiModalPreTraining.from_pretrained(pretrained, config, compute_dtype=compute_dtype)
        self.bert_pretrained.train()

    def forward(self, input_ids, image_feat, image_loc, sep_indices=None, sep_len=None, token_type_ids=None,
                token_position_ids=None, attention_mask=None, masked_lm_labels=None, next_sentence_label=None,
                head_mask=None, random_round_indices=None, output_nsp_scores=False, output_lm_scores=False,
                image_attention_mask=None, co_attention_mask=None, image_label=None, image_target=None,
                nsp_weight=None, lm_weight=None, image_index=None, lm_advantage=None, lm_behaviour_logp=None,
                lm_objective=None, lm_reference=None, lm_preference=None, shared_context=None):
        masked_lm_loss = masked_img_loss = nsp_loss = None
        kw = dict(sep_indices=sep_indices, sep_len=sep_len, token_type_ids=token_type_ids,
                  position_ids=token_position_ids, attention_mask=attention_mask, masked_lm_labels=masked_lm_labels,
                  next_sentence_label=next_sentence_label, image_attention_mask=image_attention_mask,
                  co_attention_mask=co_attention_mask, image_label=image_label, image_target=image_target,
                  nsp_weight=nsp_weight, lm_weight=lm_weight, _want_lm_scores=output_lm_scores, image_index=image_index,
                  lm_advantage=lm_advantage, lm_behaviour_logp=lm_behaviour_logp, lm_objective=lm_objective,
                  lm_reference=lm_reference, lm_preference=lm_preference, shared_context=shared_context)
        if shared_context is not None or (next_sentence_label is not None and masked_lm_labels is not None and image_target is not None):
            masked_lm_loss, masked_img_loss, nsp_loss, _, prediction_scores_t, seq_relationship_score = \
                self.bert_pretrained(input_ids, image_feat, image_loc, **kw)
        else:
            prediction_scores_t, _, seq_relationship_score, _, _ = \
                self.bert_pretrained(input_ids, image_feat, image_loc, _want_pred_v=False, **kw)
        out = (masked_lm_loss, masked_img_loss, nsp_loss)
        if output_nsp_scores:
            out = out + (seq_relationship_score,)
        if output_lm_scores:
            out = out + (prediction_scores_t,)
        return out

    def generate_answers(self, input_ids, image_feat, image_loc, context_len, token_type_ids=None, position_ids=None,
                         image_attention_mask=None, image_index=None, *, beams=1, max_answer_len=20, min_answer_len=1,
                         length_penalty=0.0, banned_tokens=(0, 101, 103), samples=0, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                         sample_streams=None, greedy=False, no_repeat_ngram_size=0, repetition_penalty=1.0, repeat_scope="answer",
                         ensemble=None, ensemble_weights=None, ensemble_mode="prob", plausibility=0.0, draft_accept="match",
                         draft=None, draft_len=4):
        """BertForMultiModalPreTraining.generate_answers."""
        return self.bert_pretrained.generate_answers(
            input_ids, image_feat, image_loc, context_len, token_type_ids, position_ids, image_attention_mask, image_index,
            beams=beams, max_answer_len=max_answer_len, min_answer_len=min_answer_len, length_penalty=length_penalty,
            banned_tokens=banned_tokens, samples=samples, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
            sample_streams=sample_streams, greedy=greedy, no_repeat_ngram_size=no_repeat_ngram_size,
            repetition_penalty=repetition_penalty, repeat_scope=repeat_scope, draft_accept=draft_accept, draft=draft,
            draft_len=draft_len, ensemble=ensemble, ensemble_weights=ensemble_weights, ensemble_mode=ensemble_mode,
            plausibility=plausibility)

    def forward_backward(self, input_ids, image_feat, image_loc, loss_weights, sep_indices=None, sep_len=None, token_type_ids=None,
                         token_position_ids=None, attention_mask=None, masked_lm_labels=None, next_sentence_label=None,
                         image_attention_mask=None, co_attention_mask=None, image_label=None, image_target=None,
                         nsp_weight=None, lm_weight=None, image_index=None, plan_header=None, lm_advantage=None,
                         lm_behaviour_logp=None, lm_objective=None, shared_context=None, lm_reference=None, lm_preference=None):
        """forward + `(c_lm * lm + c_nsp * nsp + c_img * img).backward()` in one call, loss_weights = (c_lm, c_nsp, c_img)
        (BertForMultiModalPreTraining.forward_backward, shared_context included).  -> (loss, lm_loss, img_loss, nsp_loss, nsp_logits)."""
        return self.bert_pretrained.forward_backward(
            input_ids, image_feat, image_loc, loss_weights, sep_indices=sep_indices, sep_len=sep_len, token_type_ids=token_type_ids,
            position_ids=token_position_ids, attention_mask=attention_mask, image_attention_mask=image_attention_mask,
            co_attention_mask=co_attention_mask, masked_lm_labels=masked_lm_labels, image_label=image_label, image_target=image_target,
            next_sentence_label=next_sentence_label, nsp_weight=nsp_weight, lm_weight=lm_weight, image_index=image_index,
            plan_header=plan_header, lm_advantage=lm_advantage, lm_behaviour_logp=lm_behaviour_logp, lm_objective=lm_objective,
            shared_context=shared_context, lm_reference=lm_reference, lm_preference=lm_preference)
