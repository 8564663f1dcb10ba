"""Float64 restatement of the knowledge-distillation rows (include/unimm_hip.h: unimm_distill_loss_fwd / _bwd) -- TEST
INFRASTRUCTURE, the reference of tests/test_distill_cpu.py and tests/test_gpu_distill_*.py -- and an fp32 restatement of the
forward in the kernel's operation order (`forward_f32`), which the error budgets of tests/test_gpu_distill_edges.py are held
against on the CPU.

Per row with student logits z, teacher logits zr, label y (-1 = ignore), integer weight w, temperature tau, hard share alpha:

    lse = log sum_i e^z_i,  logp = z_y - lse,  rownll = -logp (0 where y < 0)
    hard    = -w logp (w > 0);  -log(max(1 - p_y, 1e-6)) (w == -1)
    lse_t = log sum_i e^(z_i / tau),  ref_lse_t = log sum_i e^(zr_i / tau),  p = e^(z / tau - lse_t),  q = e^(zr / tau - ref_lse_t)
    KD      = sum_i q_i (log q_i - log p_i)                     (q_i = 0 contributes 0, whatever z_i holds)
    rowloss = alpha hard + (1 - alpha) tau^2 KD
    grad_i  = gs (alpha hard'_i + (1 - alpha) tau (p_i - q_i)),  hard'_i = c (softmax(z)_i - [i == y]),  c = w (w > 0);
              c = -p_y / (1 - p_y) where 1 - p_y >= 1e-6, else 0 (w == -1)
    a row takes part when y >= 0 and (w > 0 or w == -1); otherwise rowloss = KD = 0 and a zero gradient row
    nothing flows into zr
"""
import numpy as np

CLAMP = 1e-6


def _lse(x):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = x.max(1, keepdims=True)
        return (m + np.log(np.exp(x - m).sum(1, keepdims=True)))[:, 0]


def forward(z, zr, y, w, tau, alpha):
    """z, zr float [n, V] (may hold -inf), y, w int [n] -> dict of float64 arrays (per row; p1, p, q, dk per element)."""
    z, zr = np.asarray(z, np.float64), np.asarray(zr, np.float64)
    y, w = np.asarray(y).astype(np.int64), np.asarray(w).astype(np.int64)
    n = z.shape[0]
    has = y >= 0
    part = has & ((w > 0) | (w == -1))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lse = _lse(z)
        p1 = np.exp(z - lse[:, None])                                   # softmax(z): the hard term's
        logp = np.where(has, (z - lse[:, None])[np.arange(n), np.where(has, y, 0)], 0.0)
        py = np.exp(logp)
        hard = np.where(w > 0, -logp * w, np.where(w == -1, -np.log(np.maximum(1.0 - py, CLAMP)), 0.0))
        lse_t, ref_lse_t = _lse(z / tau), _lse(zr / tau)
        lp, lq = z / tau - lse_t[:, None], zr / tau - ref_lse_t[:, None]
        p, q = np.exp(lp), np.exp(lq)
        live = q > 0
        dk = np.where(live, lq - lp, 0.0)
        kd_raw = np.where(live, q * dk, 0.0).sum(1)
        adiff = np.where(live, q * np.abs(zr - z), 0.0).sum(1) / tau    # sum_i q_i |zr_i - z_i| / tau (KD's allowance)
        # (a share of 0 adds nothing: the hard term is +inf on a -inf label, the KD +inf on the row outside the -inf contract)
        rowloss = np.where(part, (alpha * hard if alpha != 0 else 0.0) + ((1.0 - alpha) * tau * tau * kd_raw if alpha != 1 else 0.0), 0.0)
    return dict(lse=lse, lse_t=lse_t, ref_lse_t=ref_lse_t, p1=p1, p=p, q=q, logp=logp, py=py, hard=np.where(part, hard, 0.0),
                kd_raw=kd_raw, kd=np.where(part, kd_raw, 0.0), adiff=adiff, rowloss=rowloss, rownll=np.where(has, -logp, 0.0),
                has=has, part=part, tau=float(tau), alpha=float(alpha))


def hard_coef(fw, w):
    """the hard term's coefficient c per row (before alpha and gs): w, or the unlikelihood's -p_y / (1 - p_y), 0 once clamped"""
    w = np.asarray(w).astype(np.int64)
    om = 1.0 - fw["py"]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(w > 0, w.astype(np.float64), np.where((w == -1) & (om >= CLAMP), -fw["py"] / np.where(om > 0, om, 1.0), 0.0))
    return np.where(fw["part"], c, 0.0)


def backward(fw, y, w, gs):
    """fw = forward(...) -> (grad [n, V], the hard term, the soft term) in float64."""
    n, V = fw["p"].shape
    onehot = np.zeros((n, V))
    has = fw["has"]
    onehot[np.nonzero(has)[0], np.asarray(y)[has]] = 1.0
    tau, alpha = fw["tau"], fw["alpha"]
    g_hard = gs * alpha * hard_coef(fw, w)[:, None] * (fw["p1"] - onehot)
    g_soft = gs * (1.0 - alpha) * tau * (fw["p"] - fw["q"]) * fw["part"][:, None]
    return g_hard + g_soft, g_hard, g_soft


def torch_objective(z, zr, y, w, tau, alpha):
    """The same objective composed of torch's own ops on float64 tensors -> the sum of the rows' losses (finite logits only)."""
    import torch
    import torch.nn.functional as F
    y = torch.as_tensor(np.asarray(y)).long()
    w = torch.as_tensor(np.asarray(w)).long()
    part = (y >= 0) & ((w > 0) | (w == -1))
    logp = torch.log_softmax(z, -1).gather(1, y.clamp_min(0)[:, None])[:, 0]
    hard = torch.where(w > 0, -logp * w.double(), -torch.log(torch.clamp(1.0 - logp.exp(), min=CLAMP)))
    kd = F.kl_div(torch.log_softmax(z / tau, -1), torch.log_softmax(zr.detach() / tau, -1), log_target=True, reduction="none").sum(-1)
    row = alpha * hard + (1.0 - alpha) * tau * tau * kd
    return torch.where(part, row, torch.zeros_like(row)).sum()


# ---------------------------------------------------------------------------------------------------------------------------
# the forward in fp32, in the kernel's order of operations (csrc/distill.hip: row_stats): 256 lanes, the 4096-float unrolled
# step, the 1024-float step, the scalar tail, the wave butterflies and the four-wave sums.  numpy's fp32 exp and log stand in
# for the device's.
# ---------------------------------------------------------------------------------------------------------------------------
F = np.float32
NINF = F(-np.inf)


def _exp(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(x.astype(F)).astype(F)


class _Lanes:
    def __init__(self, n, it):
        self.it = F(it)
        self.m, self.mr = np.full((n, 256), NINF, F), np.full((n, 256), NINF, F)
        self.s, self.st, self.sr, self.ur = (np.zeros((n, 256), F) for _ in range(4))

    def step(self, a, r, on):
        """a, r [n, 256, k] (k = 16, 4 or 1 columns of each lane, in the kernel's order), on [256]: the lanes that take the step"""
        it = self.it
        with np.errstate(invalid="ignore", over="ignore"):
            mm = a.max(2)
            up = on[None, :] & (mm > self.m)
            d = np.where(up, self.m - mm, F(0)).astype(F)
            self.s = np.where(up, self.s * _exp(d), self.s).astype(F)
            self.st = np.where(up, self.st * _exp((d * it).astype(F)), self.st).astype(F)
            self.m = np.where(up, mm, self.m)
            mq = r.max(2)
            upr = on[None, :] & (mq > self.mr)
            f = _exp((np.where(upr, self.mr - mq, F(0)).astype(F) * it).astype(F))
            self.sr = np.where(upr, self.sr * f, self.sr).astype(F)
            self.ur = np.where(upr, self.ur * f, self.ur).astype(F)
            self.mr = np.where(upr, mq, self.mr)
            for u in range(0, a.shape[2], 4):
                k = min(4, a.shape[2] - u)
                au, ru = a[:, :, u:u + k], r[:, :, u:u + k]
                e = np.where(au > NINF, _exp((au - self.m[:, :, None]).astype(F)), F(0))
                et = np.where(au > NINF, _exp(((au - self.m[:, :, None]).astype(F) * it).astype(F)), F(0))
                q = np.where(ru > NINF, _exp(((ru - self.mr[:, :, None]).astype(F) * it).astype(F)), F(0))
                uu = np.where(ru > NINF, (q * (ru - au).astype(F)).astype(F), F(0))

                def chain(x):
                    acc = x[:, :, 0]
                    for j in range(1, k):
                        acc = (acc + x[:, :, j]).astype(F)
                    return acc
                for name, x in (("s", e), ("st", et), ("sr", q), ("ur", uu)):
                    setattr(self, name, np.where(on[None, :], (getattr(self, name) + chain(x)).astype(F), getattr(self, name)).astype(F))


def _block_sum(v):
    n = v.shape[0]
    v = v.reshape(n, 4, 64).astype(F)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, :, lane ^ o]).astype(F)
    r = v[:, :, 0]
    return (((r[:, 0] + r[:, 1]).astype(F) + r[:, 2]).astype(F) + r[:, 3]).astype(F)


def forward_f32(z, zr, tau, vec=True):
    """z, zr float32 [n, V], vec: whether the student row's stride is a multiple of 4 floats -> lse, lse_t, ref_lse_t, kd (fp32 [n])"""
    z, zr = np.asarray(z, F), np.asarray(zr, F)
    n, V = z.shape
    tau = F(tau)
    it = (F(1) / tau).astype(F)
    L = _Lanes(n, it)
    t = np.arange(256)

    def cols(idx):                                                       # idx [256, k] column indices (-1: no column)
        ok = idx >= 0
        a = np.where(ok[None], z[:, np.where(ok, idx, 0)], NINF)
        r = np.where(ok[None], zr[:, np.where(ok, idx, 0)], NINF)
        return a.astype(F), r.astype(F)

    nv = (V >> 2) if vec else 0
    i = t.copy()
    while (i + 768 < nv).any():
        on = i + 768 < nv
        g = i[:, None] + 256 * np.arange(4)[None, :]                     # the lane's four groups
        idx = (4 * g[:, :, None] + np.arange(4)[None, None, :]).reshape(256, 16)
        L.step(*cols(np.where(on[:, None], idx, -1)), on)
        i = np.where(on, i + 1024, i)
    while (i < nv).any():
        on = i < nv
        idx = 4 * i[:, None] + np.arange(4)[None, :]
        L.step(*cols(np.where(on[:, None], idx, -1)), on)
        i = np.where(on, i + 256, i)
    i = (nv << 2) + t
    while (i < V).any():
        on = i < V
        L.step(*cols(np.where(on, i, -1)[:, None]), on)
        i = i + 256
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        gm = L.m.max(1)
        dead = L.m == NINF
        gs = _block_sum(np.where(dead, F(0), L.s * _exp((L.m - gm[:, None]).astype(F))))
        gst = _block_sum(np.where(dead, F(0), L.st * _exp(((L.m - gm[:, None]).astype(F) * it).astype(F))))
        lse = (gm + np.log(gs).astype(F)).astype(F)
        lse_t = (gm.astype(np.float64) * np.float64(it) + np.log(gst).astype(F).astype(np.float64)).astype(F)      # one fma
        gmr = L.mr.max(1)
        deadr = L.mr == NINF
        fr = _exp(((L.mr - gmr[:, None]).astype(F) * it).astype(F))
        gsr = _block_sum(np.where(deadr, F(0), L.sr * fr))
        gur = _block_sum(np.where(deadr, F(0), L.ur * fr))
        ref_lse_t = (gmr.astype(np.float64) * np.float64(it) + np.log(gsr).astype(F).astype(np.float64)).astype(F)
        kd = (((gur / (gsr * tau).astype(F)).astype(F) - ref_lse_t).astype(F) + lse_t).astype(F)
    return lse, lse_t, ref_lse_t, kd


# ---------------------------------------------------------------------------------------------------------------------------
# the error budgets of tests/test_gpu_distill_edges.py (derived in its docstring), from the float64 reference's quantities only
# ---------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24


def allowances(fw, z, zr, y, w, gs):
    """fw = forward(...) -> dict: A (lse), At / Art (lse_t / ref_lse_t), EKD (kd), loss (rowloss, absolute), abs_err (gradient)"""
    z, zr = np.asarray(z, np.float64), np.asarray(zr, np.float64)
    y, w = np.asarray(y).astype(np.int64), np.asarray(w).astype(np.int64)
    tau, alpha, has, part = fw["tau"], fw["alpha"], fw["has"], fw["part"]
    n, V = z.shape
    A = U * (256 + 4 * np.abs(fw["lse"]))
    At = U * (320 + 6 * np.abs(fw["lse_t"]))
    Art = U * (320 + 6 * np.abs(fw["ref_lse_t"]))
    EKD = U * (640 + 8 * np.abs(fw["lse_t"]) + 8 * np.abs(fw["ref_lse_t"]) + 864 * fw["adiff"])
    # the hard term: tests/test_gpu_row_edges.py's allowances (lm_gates), in absolute terms
    T = U * (16 + 4 * np.abs(fw["lse"]))
    om = np.where(has, 1.0 - fw["py"], 1.0)
    canc = (T * fw["py"] + 2 * U) / np.maximum(om, 1e-300)
    ul = (w == -1) & has & (om >= CLAMP)
    with np.errstate(invalid="ignore"):
        hard = np.where(np.isfinite(fw["hard"]), fw["hard"], 0.0)
        hard_allow = np.where(w > 0, w * A, np.where(ul, 2 * canc, 0.0)) + 1e-6 * np.abs(hard)
        loss = alpha * hard_allow + (1.0 - alpha) * tau * tau * EKD + 1e-6 * np.abs(np.where(np.isfinite(fw["rowloss"]), fw["rowloss"], 0.0))
    onehot = np.zeros((n, V))
    onehot[np.nonzero(has)[0], y[has]] = 1.0
    c = np.abs(gs * alpha * hard_coef(fw, w))
    abs_hard = c * (2 * (A * fw["p1"].max(1) + 2 * U) + np.where(ul, 2 * canc * np.abs(fw["p1"] - onehot).max(1), 0.0))
    p, q = fw["p"], fw["q"]
    with np.errstate(invalid="ignore", divide="ignore"):
        ep = np.where(p > 0, p * (At[:, None] + U * (np.abs(np.log(p)) + np.abs(z) / tau + 4)), 0.0)
        eq = np.where(q > 0, q * (Art[:, None] + U * (np.abs(np.log(q)) + np.abs(zr) / tau + 4)), 0.0)
    abs_soft = abs(gs * (1.0 - alpha) * tau) * (ep + eq).max(1) * part
    return dict(A=A, At=At, Art=Art, EKD=EKD, loss=loss, abs_err=abs_hard + abs_soft, ul=ul, zero_coef=(c == 0) & ((alpha == 1) | ~part))
