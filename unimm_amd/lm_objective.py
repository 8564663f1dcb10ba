"""What one step does with the LM head's fp32 logits rows: one class per objective, bound once per call.

`policy.bind_objective` makes one from the `lm_*` keywords of `forward` / `forward_backward` (None: the likelihood step,
`LIKELIHOOD`); the engine's `inp` carries it under `KEY`, `Engine._lm_head` moves it into the head's state, lm["objective"]:
    stage(pos, dev)               its per-token inputs to the device; pos: the decoded rows' flat positions b * T + t, int32
    forward(eng, lm, n, n_dev)    the row kernels on lm["logits" / "labels" / "weights"] -> lm["rowloss" / "rownll" / "lse"] (+ "ent",
                                  "kl", "ref_lse"; "lse_t", "ref_lse_t", "kd"); n, n_dev: the rows' capacity and, on the replicated
                                  schedule, device-side count
    loss(eng, lm)                 the fp32 [1] LM loss; sets the engine's last_lm_* reports
    backward(eng, lm, g, dlog)    fills dlog, the loss gradient w.r.t. the logits rows (`Engine._lm_loss_grad`)
    reference                     the frozen model whose forward the step needs first (`Engine._reference_rows`: `.ref`), or None"""
from __future__ import annotations

import torch

from . import lib as L

F32 = torch.float32
KEY = "lm_bound"
REPORTS = ("last_lm_entropy",        # engine attributes: fp32 [1], mean entropy of the rows the last policy-gradient step trained
           "last_lm_kl",             # fp32 [1]: mean KL(p || p_ref) of those rows when the step had a reference (kl_coef > 0)
           "last_lm_preference",     # the last preference step's device tensors: seq_score, seq_prob, group_loss, adv, row_seq
           "last_lm_distill")        # fp32 [1]: mean KL(teacher || student) at the temperature of the rows the last distillation step trained


def _row_mean(lm, key):                        # sum(lm[key]) over the step's rows / their number, fp32 [1]
    out = torch.empty(1, dtype=F32, device=lm[key].device)
    L.reduce_sum(lm[key], lm["n"], out, 1.0 / lm["n"], n_dev=lm.get("n_dev"), scale_dev=lm.get("inv_dev"))
    return out


def _same_rows(ref, n):
    if ref.shape[0] != n:
        raise L.UnimmHipError(f"the reference decoded {ref.shape[0]} rows, the policy {n}: not the same step's rows")


class Likelihood:
    """The weighted likelihood / unlikelihood of the labelled rows.  Stateless: `LIKELIHOOD` serves every step."""
    reference = None

    def stage(self, pos, dev):
        pass

    def forward(self, eng, lm, n, n_dev):
        L.lm_loss_fwd(lm["logits"], lm["labels"], lm["weights"], lm["rowloss"], lm["rownll"], lm["lse"], n, eng.cfg.vocab_size,
                      n_dev=n_dev)

    def loss(self, eng, lm):
        return _row_mean(lm, "rowloss")

    def backward(self, eng, lm, g, dlog):
        L.lm_loss_bwd(lm["logits"], lm["labels"], lm["weights"], lm["lse"], g, 1.0 / lm["n"], dlog, lm["n"], eng.cfg.vocab_size,
                      n_dev=lm.get("n_dev"), inv_dev=lm.get("inv_dev"))


LIKELIHOOD = Likelihood()


class PolicyGradient:
    """The advantage-weighted objective on sampled answers (unimm_pg_loss_*), entropy kept with lse; with `reference` (the
    objective has kl_coef > 0) the penalty against the reference's rows `ref` as well (unimm_pg_kl_loss_*)."""

    def __init__(self, advantage, behaviour_logp, objective, reference=None):
        self.objective, self.reference, self.ref, self.pos = objective, reference, None, None
        self.mode = L.PG_RATIO if objective.mode == "ratio" else L.PG_LOGP
        self.adv, self.blogp = advantage, behaviour_logp if self.mode == L.PG_RATIO else None      # [B, T]; staged: fp32 [B * T]
        self.eps, self.beta, self.kl_coef = float(objective.clip_eps), float(objective.entropy_coef), float(objective.kl_coef)

    def stage(self, pos, dev):
        flat = lambda t: t.to(dev, dtype=F32, non_blocking=True).contiguous().reshape(-1)
        self.pos, self.adv, self.blogp = pos, flat(self.adv), None if self.blogp is None else flat(self.blogp)

    def _args(self, lm):
        return lm["logits"], lm["labels"], self.pos, self.adv, self.blogp, self.mode, self.eps, self.beta

    def forward(self, eng, lm, n, n_dev):
        rows = ("ent",) if self.ref is None else ("ent", "kl", "ref_lse")
        lm.update((k, torch.empty(n, dtype=F32, device=lm["logits"].device)) for k in rows)
        args = (*self._args(lm), lm["rowloss"], lm["rownll"], lm["lse"], lm["ent"], n, eng.cfg.vocab_size)
        if self.ref is None:
            return L.pg_loss_fwd(*args, n_dev=n_dev)
        _same_rows(self.ref, n)
        L.pg_kl_loss_fwd(*args, self.ref, self.kl_coef, lm["kl"], lm["ref_lse"], n_dev=n_dev)

    def loss(self, eng, lm):
        loss = _row_mean(lm, "rowloss")
        eng.last_lm_entropy = _row_mean(lm, "ent")         # the mean entropy of the rows the step trained
        eng.last_lm_kl = _row_mean(lm, "kl") if "kl" in lm else None           # ... and, with a reference, their mean KL to it
        return loss

    def backward(self, eng, lm, g, dlog):
        tail = dict(n_dev=lm.get("n_dev"), inv_dev=lm.get("inv_dev"))
        args = (*self._args(lm), lm["lse"], lm["ent"], g, 1.0 / lm["n"], dlog, lm["n"], eng.cfg.vocab_size)
        if self.ref is None:
            return L.pg_loss_bwd(*args, **tail)
        L.pg_kl_loss_bwd(*args, self.ref, self.kl_coef, lm["kl"], lm["ref_lse"], **tail)
        self.ref.record_stream(torch.cuda.current_stream())
        self.ref = None                        # the reference's logits are released here: the backward was their last reader


class Distillation:
    """Token-level knowledge distillation (unimm_distill_loss_*): the weighted likelihood of the labelled rows, share alpha, mixed
    with tau^2 KL(teacher || student) at temperature tau against the frozen teacher's rows `ref`.  With alpha == 1 nothing of the
    teacher is read, so `reference` is None and its forward does not run."""

    def __init__(self, objective, reference):
        self.objective, self.ref = objective, None
        self.tau, self.alpha = float(objective.temperature), float(objective.alpha)
        self.reference = reference if self.alpha != 1.0 else None

    def stage(self, pos, dev):
        pass

    def forward(self, eng, lm, n, n_dev):
        lm.update((k, torch.empty(n, dtype=F32, device=lm["logits"].device)) for k in ("lse_t", "ref_lse_t", "kd"))
        if self.ref is not None:
            _same_rows(self.ref, n)
        L.distill_loss_fwd(lm["logits"], lm["labels"], lm["weights"], self.ref, self.tau, self.alpha, lm["rowloss"], lm["rownll"],
                           lm["lse"], lm["lse_t"], lm["ref_lse_t"], lm["kd"], n, eng.cfg.vocab_size, n_dev=n_dev)

    def loss(self, eng, lm):
        loss = _row_mean(lm, "rowloss")
        # the mean KD of the rows that took part (a label and a weight > 0 or -1): two sums and a division, all on the device
        y, w, n = lm["labels"][:lm["n"]], lm["weights"][:lm["n"]], lm["n"]
        part = ((y >= 0) & ((w > 0) | (w == -1))).to(F32)
        sums = torch.empty(2, dtype=F32, device=part.device)
        L.reduce_sum(lm["kd"], n, sums[0:1], 1.0, n_dev=lm.get("n_dev"))
        L.reduce_sum(part, n, sums[1:2], 1.0, n_dev=lm.get("n_dev"))
        eng.last_lm_distill = sums[0:1] / sums[1:2]
        return loss

    def backward(self, eng, lm, g, dlog):
        L.distill_loss_bwd(lm["logits"], lm["labels"], lm["weights"], self.ref, self.tau, self.alpha, lm["lse"], lm["lse_t"],
                           lm["ref_lse_t"], g, 1.0 / lm["n"], dlog, lm["n"], eng.cfg.vocab_size, n_dev=lm.get("n_dev"),
                           inv_dev=lm.get("inv_dev"))
        if self.ref is not None:
            self.ref.record_stream(torch.cuda.current_stream())
            self.ref = None                    # the teacher's logits are released here: the backward was their last reader


class Preference(Likelihood):
    """The listwise preference over whole candidate answers (unimm_seq_pref): likelihood rows with weight 1, then per-sequence
    scores and each group's softmax against its target weights; the backward is the policy-gradient kernel's LOGP form with
    one coefficient per row.  `reference` is optional (without one log pi_ref = 0)."""

    def __init__(self, targets, objective, T, reference=None):
        self.objective, self.T, self.reference, self.ref = objective, int(T), reference, None
        self.group, self.weight, self.groups = targets.group, targets.weight, int(targets.groups)   # host arrays until staged
        self.beta, self.lnorm = float(objective.beta), bool(objective.length_normalize)

    def stage(self, pos, dev):
        self.group = torch.as_tensor(self.group).to(dev, dtype=torch.int32, non_blocking=True).contiguous().reshape(-1)
        self.weight = torch.as_tensor(self.weight).to(dev, dtype=F32, non_blocking=True).contiguous().reshape(-1)
        self.row_seq = (pos // self.T).to(torch.int32)     # the decoded rows' sequences

    def forward(self, eng, lm, n, n_dev):
        super().forward(eng, lm, n, n_dev)
        dev = lm["logits"].device
        ref, self.ref, ref_rownll = self.ref, None, None
        if ref is not None:                    # the reference's rows go through the same likelihood kernel and are released:
            _same_rows(ref, n)                 # the backward does not read them
            scratch, ref_rownll, ref_lse = (torch.empty(n, dtype=F32, device=dev) for _ in range(3))
            L.lm_loss_fwd(ref, lm["labels"], lm["weights"], scratch, ref_rownll, ref_lse, n, eng.cfg.vocab_size, n_dev=n_dev)
            ref.record_stream(torch.cuda.current_stream())
            del ref
        B, G = self.group.numel(), self.groups
        self.adv = torch.zeros(n, dtype=F32, device=dev)   # one coefficient per row
        seq_score, seq_prob = torch.empty(B, dtype=F32, device=dev), torch.empty(B, dtype=F32, device=dev)
        self.group_loss, self.alive_inv = torch.empty(G, dtype=F32, device=dev), torch.empty(1, dtype=F32, device=dev)
        L.seq_pref(lm["rownll"], ref_rownll, self.row_seq, n, self.group, self.weight, G, self.beta, self.lnorm, self.adv, seq_score,
                   seq_prob, self.group_loss, self.alive_inv, n_dev=n_dev)
        eng.last_lm_preference = dict(seq_score=seq_score, seq_prob=seq_prob, group_loss=self.group_loss, adv=self.adv,
                                      row_seq=self.row_seq)

    def loss(self, eng, lm):                   # sum(group_loss) / #alive (NaN when no group is alive)
        loss = torch.empty(1, dtype=F32, device=self.group_loss.device)
        L.reduce_sum(self.group_loss, self.groups, loss, 1.0, scale_dev=self.alive_inv)
        return loss

    def backward(self, eng, lm, g, dlog):
        # -(c_j / #alive)(onehot_y - p): LOGP rows with A = c_j, the denominator word #alive
        L.pg_loss_bwd(lm["logits"], lm["labels"], None, self.adv, None, L.PG_LOGP, 0.0, 0.0, lm["lse"], lm["lse"], g, 1.0, dlog,
                      lm["n"], eng.cfg.vocab_size, n_dev=lm.get("n_dev"), inv_dev=self.alive_inv)
