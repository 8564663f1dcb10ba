"""Float64 restatement of the KL-regularised policy-gradient rows (include/unimm_hip.h: unimm_pg_kl_loss_fwd / _bwd), built on
tests/policy_ref.py -- TEST INFRASTRUCTURE, the reference of tests/test_policy_kl_cpu.py and tests/test_gpu_policy_kl_*.py.

Per row, next to what policy_ref states, with the frozen reference's logits zr and pr = softmax(zr):

    ref_lse = log sum_i e^zr_i
    KL      = sum_i p_i (log p_i - log pr_i)                    (p_i = 0 contributes 0, whatever zr_i holds)
    rowloss = policy_ref's + kl_coef KL;  y < 0: rowloss = KL = 0 and a zero gradient row
    grad_i  = policy_ref's + gs kl_coef p_i (log p_i - log pr_i - KL)
    nothing flows into zr
"""
import numpy as np

from tests import policy_ref as PR

LOGP, RATIO = PR.LOGP, PR.RATIO


def forward(z, zr, y, A, b, mode, eps, beta, kl_coef):
    """policy_ref.forward(z, ...) plus: ref_lse, kl (0 on ignored rows), kl_raw (every row), dk [n, V] = log p - log pr where
    p > 0 (0 elsewhere), adiff = sum_i p_i |z_i - zr_i| (the KL's allowance), rowloss with the penalty."""
    fw = PR.forward(z, y, A, b, mode, eps, beta)
    z = np.asarray(z, np.float64)
    zr = np.asarray(zr, np.float64)
    p, lp = fw["p"], fw["lp_all"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mr = zr.max(1, keepdims=True)
        ref_lse = (mr + np.log(np.exp(zr - mr).sum(1, keepdims=True)))[:, 0]
        live = p > 0
        dk = np.where(live, lp - (zr - ref_lse[:, None]), 0.0)
        kl_raw = np.where(live, p * dk, 0.0).sum(1)
        adiff = np.where(live, p * np.abs(z - zr), 0.0).sum(1)
    has = fw["has"]
    fw.update(ref_lse=ref_lse, kl_raw=kl_raw, kl=np.where(has, kl_raw, 0.0), dk=dk, adiff=adiff, kl_coef=float(kl_coef),
              rowloss_pg=fw["rowloss"])
    fw["rowloss"] = np.where(has, fw["rowloss"] + (kl_coef * kl_raw if kl_coef != 0 else 0.0), 0.0)
    return fw


def backward(fw, y, beta, gs):
    """fw = forward(...) -> (grad [n, V], the advantage term, the entropy term, the KL term) in float64."""
    grad, g_adv, g_ent = PR.backward(fw, y, beta, gs)
    p = fw["p"]
    with np.errstate(invalid="ignore"):
        g_kl = gs * fw["kl_coef"] * np.where(p > 0, p * (fw["dk"] - fw["kl_raw"][:, None]), 0.0) * fw["has"][:, None]
    return grad + g_kl, g_adv, g_ent, g_kl


def torch_objective(z, zr, y, A, b, mode, eps, beta, kl_coef):
    """The same objective with torch ops on float64 tensors z, zr -> sum of the rows' losses (finite logits only).  The
    reference is frozen: its logits enter detached, so no gradient reaches zr even when it requires grad."""
    import torch
    base = PR.torch_objective(z, y, A, b, mode, eps, beta)
    has = torch.as_tensor(np.asarray(y)).long() >= 0
    lsm, lsr = torch.log_softmax(z, -1), torch.log_softmax(zr.detach(), -1)
    kl = (lsm.exp() * (lsm - lsr)).sum(-1)
    return base + kl_coef * torch.where(has, kl, torch.zeros_like(kl)).sum()
