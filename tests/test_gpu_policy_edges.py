"""unimm_pg_loss_fwd / unimm_pg_loss_bwd per element against the float64 restatement (tests/policy_ref.py), on rows built like
the `lm_logits` kinds of tests/test_gpu_row_edges.py (normal, one dominant logit, huge magnitudes, flat) plus rows with -inf
logits off and on the label, at every (V, ld) at which the kernels take another path, and at every edge a device-side row
count can sit on.  The gates are per row (rows_ref.row_ratio) and printed next to their worst ratio, as in that file.

Allowances (U = 2^-24; every quantity below is the float64 reference's, none is read from the kernel's output):

  * lse, rownll, the LOGP rowloss: that file's.  A = U (256 + 4 |lse|) absolute for lse, A + 1e-6 |nll| for rownll,
    |adv| A + 1e-6 |loss| for the rowloss.
  * the importance ratio r = exp(logp - b): logp carries A, its rounding U |logp|, the subtraction U |logp - b|, b itself is an
    fp32 number (U |b|), expf 2 U more:  rho = A + U (|logp| + |logp - b| + |b| + 4)  relative.  The RATIO rowloss gets
    |adv| r rho + 1e-6 |loss|, the RATIO gradient |c| rho max|p - onehot| on top of the LOGP gradient's allowance.
  * the entropy, H = lse - t / s with s = sum e^(z_i - m) and t = sum e^(z_i - m) z_i accumulated side by side.  That file budgets
    256 roundings for the fp32 sum s (the 256 of A: a lane adds ceil(V / 256) <= 120 terms, the wave and block trees 8 levels,
    expf and the rescaling by e^(m - m') a few each).  t is accumulated in the same order with one more rounding per term (the
    product), so  |dt| <= 257 U sum e |z|  and  |ds| <= 256 U s;  t / s = sum p_i z_i  is therefore off by at most
    (257 + 256 + 1) U sum p_i |z_i|  (the + 1: the division), and the final subtraction rounds once more, U |H| <= U (|lse| +
    sum p_i |z_i|).  With the error of lse itself:
        E_H = U (256 + 5 |lse| + 516 sum_i p_i |z_i|)   absolute.
    When one logit dominates, H is a difference of two numbers of size |lse| and E_H can exceed H itself: such rows (E_H >
    2^-10 |H|) are gated by the same E_H but reported apart, as that file does for 1 - p_y.  The rowloss gets beta E_H on top.
  * the gradient: bf16 rounding of the element (BF) + fp32 slack (F32) + gx, all relative to the row's largest |reference|,
    where gx is the sum of the following absolute errors divided by that largest |reference|:
        |gs c| 2 (A max p + 2 U)                          that file's grad_extra (the error of p = exp(z - lse), and p_y - 1)
        |gs c| rho max|p - onehot|                        RATIO only
        |gs beta| max_i p_i ((A + 4 U) |log p_i + H| + A + E_H)      the entropy term p_i (log p_i + H): p_i is off by (A + 4 U)
                                                          relative, log p_i by A, H by E_H
    With beta = 0 and LOGP this is that file's gate without its unlikelihood term."""
import math

import numpy as np
import pytest
import torch

from oracle import rows_ref as RR
from tests import policy_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
BF, F32 = 2.0 ** -8, 2.0 ** -14
NAN16, NAN32 = 0x7FA5, 0x7FA5A5A5
NORMAL, DOMINANT, HUGE, FLAT, NEGINF_OFF, NEGINF_ON = range(6)
ADV = (1.5, -0.75, 0.0, 2.0)
EPS = 0.2


def gate(name, ratios, limit):
    r = np.asarray(ratios, np.float64).reshape(-1)
    lim = np.broadcast_to(np.asarray(limit, np.float64), r.shape)
    if r.size == 0:
        return
    bad = ~(r <= lim)
    i = int(np.argmax(r))
    print(f"[policy-edges] {name}: worst {r[i]:.3g} (gate {lim[i]:.3g})")
    assert not bad.any(), (name, int(np.argmax(bad)), float(r[np.argmax(bad)]), float(lim[np.argmax(bad)]))


def sent16(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def sent32(*shape):
    return torch.full(shape, NAN32, dtype=torch.int32, device=DEV).view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


def f64(t):
    return t.detach().float().cpu().double().numpy()


def dword(v, dtype=torch.int32):
    return torch.tensor([v], dtype=dtype, device=DEV)


def dev(a, dtype):
    return torch.from_numpy(np.asarray(a).astype(dtype)).to(DEV)


def pg_logits(kinds, V, ld, seed):
    rng = np.random.default_rng(seed)
    n = len(kinds)
    z = np.full((n, ld), np.nan, np.float32)                        # columns V .. ld must never be read
    y = rng.integers(0, V, n)
    for i, k in enumerate(kinds):
        if k == DOMINANT:
            z[i, :V] = rng.standard_normal(V)
            z[i, y[i]] = 30.0
        elif k == HUGE:
            z[i, :V] = rng.uniform(-1e4, 1e4, V)
        elif k == FLAT:
            z[i, :V] = 5.0
        else:
            z[i, :V] = rng.standard_normal(V) * 2
            if k in (NEGINF_OFF, NEGINF_ON):                        # single columns, a whole aligned group of four, the tail
                off = rng.random(V) < 0.125
                off[:4] = True
                off[V - 1] = True
                if k == NEGINF_OFF and off.all():
                    off[:] = False
                    off[(y[i] + 1) % V] = True
                z[i, :V][off] = -np.inf
                z[i, y[i]] = -np.inf if k == NEGINF_ON else 2.0
                if k == NEGINF_ON and np.isinf(z[i, :V]).all():
                    z[i, (y[i] + 1) % V] = 1.0                        # a row keeps at least one finite logit
    return z, y


def build_rows(V, ld, seed):
    """24 rows: every kind with every advantage; three rows are unlabelled, one of them with a non-zero advantage.  The behaviour log-probabilities put r = exp(logp -
    b) below 1 - EPS, inside and above 1 + EPS for every sign of the advantage (huge rows: |logp - b| = 19.5)."""
    kinds = [k for k in range(6) for _ in ADV]
    z, y = pg_logits(kinds, V, ld, seed)
    adv = np.array([a for _ in range(6) for a in ADV], np.float32)
    for k, slot in ((NORMAL, 2), (FLAT, 3), (NEGINF_OFF, 2)):
        y[4 * k + slot] = -1
    base = PR.forward(z[:, :V], y, np.zeros(len(y)), None, PR.LOGP, math.inf, 0.0)
    shift = np.array([((-19.5, 0.1, 19.5) if kinds[i] == HUGE else (-0.5, 0.0, 0.5))[(i % 4 + 2 * (i // 4)) % 3] for i in range(len(y))])
    with np.errstate(invalid="ignore"):
        b = np.where(np.isfinite(base["logp"]), base["logp"] - shift, -3.0).astype(np.float32)
    return np.array(kinds), z, y, adv, b


def allowances(fw, gs, beta, mode, adv, b, y):
    """the docstring's allowances from the float64 reference -> dict"""
    lse, H, p, lp = fw["lse"], fw["ent"], fw["p"], fw["lp_all"]
    A = U * (256 + 4 * np.abs(lse))
    EH = U * (256 + 5 * np.abs(lse) + 516 * fw["ez"])
    logp = np.where(np.isfinite(fw["logp"]), fw["logp"], 0.0)
    rho = A + U * (np.abs(logp) + np.abs(logp - b) + np.abs(b) + 4) if mode == PR.RATIO else np.zeros_like(A)
    n, V = p.shape
    onehot = np.zeros_like(p)
    onehot[np.nonzero(fw["has"])[0], y[fw["has"]]] = 1.0
    with np.errstate(invalid="ignore"):
        ent_el = np.where(p > 0, p * ((A + 4 * U)[:, None] * np.abs(lp + H[:, None]) + (A + EH)[:, None]), 0.0).max(1)
    c = np.abs(gs * fw["c"])
    abs_err = c * 2 * (A * p.max(1) + 2 * U) + c * rho * np.abs(p - onehot).max(1) + abs(gs * beta) * ent_el * fw["has"]
    return dict(A=A, EH=EH, rho=rho, abs_err=abs_err)


CONFIGS = [(PR.LOGP, math.inf, 0.0, False), (PR.LOGP, math.inf, 0.01, True), (PR.RATIO, EPS, 0.0, True),
           (PR.RATIO, EPS, 0.01, False), (PR.RATIO, math.inf, 0.01, True)]


@pytest.mark.parametrize("V,ld", [(30522, 30522), (30522, 30528), (4100, 4100), (1000, 1001), (8, 8), (3, 4)])
def test_pg_loss_numerical_edges(V, ld):
    from unimm_amd import lib
    kinds, z, y, adv, b = build_rows(V, ld, seed=V + ld)
    n = len(y)
    rng = np.random.default_rng(V)
    pos = rng.permutation(np.arange(n) * 3 + 1)                     # a permutation with gaps: adv / blogp of 3 n + 2 entries
    adv_p, b_p = np.full(3 * n + 2, np.nan, np.float32), np.full(3 * n + 2, np.nan, np.float32)
    adv_p[pos], b_p[pos] = adv, b
    zg, yg = torch.from_numpy(z).to(DEV), dev(y, np.int32)
    g, inv = 0.75, 1.0 / 37
    gs = float(np.float32(g) * np.float32(inv))
    gdev = dword(g, torch.float32)
    ldd = (V + 7) // 8 * 8 + 8
    inf_rows = (kinds == NEGINF_OFF) | (kinds == NEGINF_ON)
    for mode, eps, beta, with_pos in CONFIGS:
        tag = f"V={V} ld={ld} mode={'ratio' if mode else 'logp'} eps={eps} beta={beta} pos={'given' if with_pos else 'NULL'}"
        fw = PR.forward(z[:, :V], y, adv, b, mode, eps, beta)
        grad_r, _, _ = PR.backward(fw, y, beta, gs)
        al = allowances(fw, gs, beta, mode, adv.astype(np.float64), b.astype(np.float64), y)
        A, EH = al["A"], al["EH"]
        pg = dev(pos, np.int32) if with_pos else None
        ag, bg = (dev(adv_p, np.float32), dev(b_p, np.float32)) if with_pos else (dev(adv, np.float32), dev(b, np.float32))
        if mode == PR.LOGP:
            bg = None                                                 # not read
        rowloss, rownll, lse, ent = sent32(n), sent32(n), sent32(n), sent32(n)
        lib.pg_loss_fwd(zg, yg, pg, ag, bg, mode, eps, beta, rowloss, rownll, lse, ent, n, V)
        dl = sent16(n, ldd)
        lib.pg_loss_bwd(zg, yg, pg, ag, bg, mode, eps, beta, lse, ent, gdev, inv, dl, n, V)
        torch.cuda.synchronize()
        got = {k: f64(t) for k, t in (("lse", lse), ("ent", ent), ("rowloss", rowloss), ("rownll", rownll))}
        gd = f64(dl)
        for k, v in got.items():
            assert not np.isnan(v).any(), (tag, k)                    # no NaN anywhere, the -inf rows included
        assert not np.isnan(gd).any(), tag
        has = fw["has"]
        gate(f"lse {tag} (abs / A)", np.abs(got["lse"] - fw["lse"]) / A, 1.0)
        cancels = EH > 2.0 ** -10 * np.abs(fw["ent"])
        gate(f"ent {tag} (abs / E_H)", (np.abs(got["ent"] - fw["ent"]) / EH)[~cancels], 1.0)
        gate(f"ent {tag} (abs / E_H, rows whose H cancels)", (np.abs(got["ent"] - fw["ent"]) / EH)[cancels], 1.0)
        fin = has & np.isfinite(fw["rownll"])
        gate(f"rownll {tag} (abs)", np.abs(got["rownll"][fin] - fw["rownll"][fin]), (A + 1e-6 * np.abs(fw["rownll"]))[fin])
        assert (got["rownll"][has & ~fin] == np.inf).all() and (got["rownll"][~has] == 0).all() and (got["rowloss"][~has] == 0).all()
        lfin = has & np.isfinite(fw["rowloss"])
        assert (got["rowloss"][has & ~lfin] == fw["rowloss"][has & ~lfin]).all()              # +-inf: -inf on the label, LOGP
        a_abs = np.abs(adv.astype(np.float64))
        loss_allow = (a_abs * fw["r"] * al["rho"] if mode == PR.RATIO else a_abs * A) + beta * EH + 1e-6 * np.abs(fw["rowloss"])
        gate(f"rowloss {tag} (abs)", np.abs(got["rowloss"][lfin] - fw["rowloss"][lfin]), loss_allow[lfin])
        den = np.abs(grad_r).max(1)
        gx = al["abs_err"] / np.where(den > 0, den, 1.0)
        r16 = RR.row_ratio(gd[:, :V], grad_r)
        tight = gx < F32
        gate(f"grad {tag}", r16[tight], (BF + F32 + gx)[tight])
        gate(f"grad {tag} (rows with a cancelling term)", r16[~tight], (BF + F32 + gx)[~tight])
        assert (bits(dl[:, V:]) == 0).all(), "dlogits columns V .. ldd must be zero"
        assert (bits(dl)[~has] == 0).all(), "an unlabelled row has an exactly zero gradient, also with beta != 0"
        assert (adv[~has] != 0).any() and (adv[~has] == 0).any()
        if mode == PR.RATIO and math.isfinite(eps):
            assert fw["clipped"].sum() >= 4 and (has & ~fw["clipped"] & (adv != 0)).sum() >= 4
            if beta == 0.0:
                assert (gd[fw["clipped"]] == 0).all(), "a clipped row has an exactly zero gradient"
        else:
            assert not fw["clipped"].any()
        assert inf_rows.sum() == 8 and np.isfinite(gd[inf_rows]).all()


CAP = 40


@pytest.mark.parametrize("count", [0, 1, CAP - 1, CAP, CAP + 7])
def test_pg_loss_device_count(count):
    """n_dev / inv_dev: rows at or past the count are neither read (NaN logits, positions that point at NaN advantages) nor
    written (sentinels survive); inv_dev overrides the host float."""
    from unimm_amd import lib
    V, ld, cap = 1000, 1004, CAP
    live = RR.live(count, cap)
    total = cap + 8
    rng = np.random.default_rng(count)
    z, y = pg_logits([NORMAL] * total, V, ld, seed=count)
    adv = rng.standard_normal(total).astype(np.float32)
    y[2::7] = -1
    base = PR.forward(z[:, :V], y, np.zeros(total), None, PR.LOGP, math.inf, 0.0)
    b = (base["logp"] - np.array([(-0.5, 0.0, 0.5)[i % 3] for i in range(total)])).astype(np.float32)
    pos = rng.permutation(np.arange(total) * 2)
    adv_p, b_p = np.full(2 * total, np.nan, np.float32), np.full(2 * total, np.nan, np.float32)
    adv_p[pos[:live]], b_p[pos[:live]] = adv[:live], b[:live]
    z[live:] = np.nan
    mode, eps, beta, inv = PR.RATIO, EPS, 0.01, 0.125
    gs = 0.5 * inv
    fw = PR.forward(z[:live, :V], y[:live], adv[:live], b[:live], mode, eps, beta)
    grad_r, _, _ = PR.backward(fw, y[:live], beta, gs)
    zg, yg, pg = torch.from_numpy(z).to(DEV), dev(y, np.int32), dev(pos, np.int32)
    ag, bg = dev(adv_p, np.float32), dev(b_p, np.float32)
    n_dev, inv_dev, gdev = dword(count), dword(inv, torch.float32), dword(0.5, torch.float32)
    outs = [sent32(total) for _ in range(4)]
    rowloss, rownll, lse, ent = outs
    lib.pg_loss_fwd(zg, yg, pg, ag, bg, mode, eps, beta, rowloss, rownll, lse, ent, cap, V, n_dev=n_dev)
    dl = sent16(total, 1008)
    lib.pg_loss_bwd(zg, yg, pg, ag, bg, mode, eps, beta, lse, ent, gdev, 99.0, dl, cap, V, n_dev=n_dev, inv_dev=inv_dev)
    torch.cuda.synchronize()
    for name, t in zip(("rowloss", "rownll", "lse", "ent"), outs):
        assert (bits(t[live:]) == NAN32).all(), f"pg_loss_fwd {name}: rows past the count are not written"
    assert (bits(dl[live:]) == np.int16(NAN16)).all(), "pg_loss_bwd: rows past the count are not written"
    if live:
        al = allowances(fw, gs, beta, mode, adv[:live].astype(np.float64), b[:live].astype(np.float64), y[:live])
        gate("(n_dev) lse (abs / A)", np.abs(f64(lse[:live]) - fw["lse"]) / al["A"], 1.0)
        gate("(n_dev) ent (abs / E_H)", np.abs(f64(ent[:live]) - fw["ent"]) / al["EH"], 1.0)
        gate("(n_dev) rowloss (abs)", np.abs(f64(rowloss[:live]) - fw["rowloss"]),
             np.abs(adv[:live]) * fw["r"] * al["rho"] + beta * al["EH"] + 1e-6 * np.abs(fw["rowloss"]))
        den = np.abs(grad_r).max(1)
        gate("(n_dev, inv_dev) grad", RR.row_ratio(f64(dl[:live, :V]), grad_r), BF + F32 + al["abs_err"] / np.where(den > 0, den, 1.0))
        assert (bits(dl[:live, V:]) == 0).all()


def test_pg_loss_refused_arguments():
    from unimm_amd import lib
    z = torch.zeros((2, 8), device=DEV)
    y = torch.zeros(2, dtype=torch.int32, device=DEV)
    adv = torch.zeros(2, device=DEV)
    o = [torch.zeros(2, device=DEV) for _ in range(4)]
    with pytest.raises(lib.UnimmHipError):                            # RATIO without behaviour log-probabilities
        lib.pg_loss_fwd(z, y, None, adv, None, lib.PG_RATIO, 0.2, 0.0, *o, 2, 8)
    with pytest.raises(lib.UnimmHipError):                            # fewer advantages than rows without positions
        lib.pg_loss_fwd(z, y, None, adv[:1], None, lib.PG_LOGP, 0.2, 0.0, *o, 2, 8)
    with pytest.raises(lib.UnimmHipError):
        lib.pg_loss_fwd(z, y, None, adv, None, 2, 0.2, 0.0, *o, 2, 8)
