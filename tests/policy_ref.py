"""Float64 restatement of the policy-gradient row objective (include/unimm_hip.h: unimm_pg_loss_fwd / unimm_pg_loss_bwd) --
TEST INFRASTRUCTURE, the only reference of tests/test_policy_cpu.py and tests/test_gpu_policy_*.py.

Per row with logits z, label y (-1 = ignore), advantage A, behaviour log-probability b:

    lse = log sum_i e^z_i,  p = e^(z - lse),  logp = z_y - lse,  H = -sum_i p_i log p_i   (p_i = 0 contributes 0)
    LOGP:   surr = A logp
    RATIO:  r = e^(logp - b),  surr = min(r A, clamp(r, 1 - eps, 1 + eps) A)
    A == 0: surr = 0 whatever logp is
    rowloss = -surr - beta H,  rownll = -logp;  y < 0: both 0 and a zero gradient row
    grad_i  = gs ( c (p_i - [i == y]) + beta p_i (log p_i + H) )
              c = A (LOGP);  c = A r (RATIO) unless the clipped branch is the strict minimum (A > 0 and r > 1 + eps, or
              A < 0 and r < 1 - eps): then c = 0
"""
import numpy as np

LOGP, RATIO = 0, 1


def forward(z, y, A, b, mode, eps, beta):
    """z float [n, V] (may hold -inf), y int [n], A / b float [n] -> dict of float64 arrays (per row; p and logp_all per element)."""
    z = np.asarray(z, np.float64)
    y = np.asarray(y).astype(np.int64)
    A = np.asarray(A, np.float64)
    b = np.zeros_like(A) if b is None else np.asarray(b, np.float64)
    n = z.shape[0]
    m = z.max(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lse = (m + np.log(np.exp(z - m).sum(1, keepdims=True)))[:, 0]
        lp_all = z - lse[:, None]
        p = np.exp(lp_all)
        ent = -np.where(p > 0, p * lp_all, 0.0).sum(1)
        ez = np.where(p > 0, p * np.abs(z), 0.0).sum(1)                  # sum_i p_i |z_i| (the entropy's allowance)
        has = y >= 0
        logp = np.where(has, lp_all[np.arange(n), np.where(has, y, 0)], 0.0)
        r = np.where(has & (mode == RATIO), np.exp(logp - b), 1.0)
        if mode == RATIO:
            lo, hi = 1.0 - eps, 1.0 + eps
            surr = np.minimum(r * A, np.clip(r, lo, hi) * A)
            clipped = ((A > 0) & (r > hi)) | ((A < 0) & (r < lo))
            c = np.where(clipped, 0.0, A * r)
        else:
            surr = A * logp
            clipped = np.zeros(n, bool)
            c = A.copy()
        surr = np.where(A == 0, 0.0, surr)
        c = np.where(has & (A != 0), c, 0.0)
        rowloss = np.where(has, -surr - (beta * ent if beta != 0 else 0.0), 0.0)
        rownll = np.where(has, -logp, 0.0)
    return dict(lse=lse, ent=ent, ez=ez, p=p, lp_all=lp_all, logp=logp, r=r, clipped=clipped & has, c=c, rowloss=rowloss,
                rownll=rownll, has=has)


def backward(fw, y, beta, gs):
    """fw = forward(...) -> (grad [n, V], its two parts: the advantage term and the entropy term) in float64."""
    p, lp_all = fw["p"], fw["lp_all"]
    n, V = p.shape
    onehot = np.zeros_like(p)
    has = fw["has"]
    onehot[np.nonzero(has)[0], np.asarray(y)[has]] = 1.0
    with np.errstate(invalid="ignore"):
        g_adv = gs * fw["c"][:, None] * (p - onehot)
        g_ent = gs * beta * np.where(p > 0, p * (lp_all + fw["ent"][:, None]), 0.0) * has[:, None]
    return g_adv + g_ent, g_adv, g_ent


def torch_objective(z, y, A, b, mode, eps, beta):
    """The same objective written with torch ops on a float64 tensor z that requires grad -> sum of the rows' losses (the
    autograd cross-check of tests/test_policy_cpu.py; finite logits only)."""
    import torch
    y = torch.as_tensor(np.asarray(y)).long()
    A = torch.as_tensor(np.asarray(A, np.float64))
    has = y >= 0
    lsm = torch.log_softmax(z, -1)
    logp = lsm.gather(1, y.clamp_min(0)[:, None])[:, 0]
    H = -(lsm.exp() * lsm).sum(-1)
    if mode == RATIO:
        r = torch.exp(logp - torch.as_tensor(np.asarray(b, np.float64)))
        surr = torch.minimum(r * A, torch.clamp(r, 1.0 - eps, 1.0 + eps) * A)
    else:
        surr = A * logp
    return torch.where(has, -surr - beta * H, torch.zeros_like(H)).sum()
