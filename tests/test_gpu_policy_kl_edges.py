"""unimm_pg_kl_loss_fwd / unimm_pg_kl_loss_bwd per element against the float64 restatement (tests/policy_kl_ref.py), on the rows
of tests/test_gpu_policy_edges.py (normal, one dominant logit, huge magnitudes, flat, -inf off and on the label) with four
kinds of reference rows, at every (V, ld, ld_ref) at which the kernels take another path -- the 4096-float unrolled step, its
remainders, the scalar tail, and a vector policy row beside a scalar reference row and the reverse -- and at every edge a
device-side row count can sit on.  The gates are per row and printed next to their worst ratio, as in that file, whose rows,
helpers and allowances (A, E_H, rho, the gradient's abs_err) are imported and used unchanged for everything the existing pair
also computes.

What the KL adds (U = 2^-24, A(x) = U (256 + 4 |x|); every quantity is the float64 reference's, none is read from the kernel):

  * ref_lse: the reference row's log-sum-exp takes the policy row's operation sequence: A(ref_lse) absolute.
  * KL = u / s - lse + ref_lse with u = sum e^(z_i - m) (z_i - zr_i) accumulated beside s and t, in their order.  That file
    budgets 256 roundings for the fp32 sum s and 257 per term for t (one more: the product).  A term of u carries one more
    rounding again (the subtraction z_i - zr_i, then the product): |du| <= 258 U sum e |z - zr|, |ds| <= 256 U s, so u / s =
    sum p_i (z_i - zr_i) is off by at most (258 + 256 + 1) U sum p_i |z_i - zr_i| = 515 U sum p_i |z_i - zr_i| (the + 1: the
    division).  The two log-sum-exps carry A(lse) and A(ref_lse).  The two final subtractions round once each: the first on a
    number of size <= sum p |z - zr| + |lse|, the second on one of size <= sum p |z - zr| + |lse| + |ref_lse|.  That adds up
    to U (512 + 6 |lse| + 5 |ref_lse| + 517 sum p |z - zr|), inside
        E_KL = U (512 + 6 |lse| + 6 |ref_lse| + 518 sum_i p_i |z_i - zr_i|)   absolute,
    the bound the kernels' specification states and the one used here.  When the two rows nearly agree KL is a difference of
    numbers of size |lse| and E_KL can exceed KL itself: such rows (E_KL > 2^-10 |KL|) are gated by the same E_KL but reported apart, as that file does for H.
  * the rowloss gets kl_coef E_KL on top of that file's allowance.
  * the gradient element gets  |gs kl_coef| p_i (log p_i - log pr_i - KL)  as its own addend: p_i is off by (A + 4 U) relative,
    log p_i - log pr_i = (z_i - lse) - (zr_i - ref_lse) by A(lse) + A(ref_lse), KL by E_KL, so that file's abs_err gets
        |gs kl_coef| max_i p_i ((A + 4 U) |log p_i - log pr_i - KL| + A(lse) + A(ref_lse) + E_KL)
    on top.  The gate is that file's -- bf16 rounding (BF) + fp32 slack (F32) relative to the row's largest |reference|, plus
    abs_err -- written in absolute terms, err <= (BF + F32) max|ref| + abs_err, because a row whose reference gradient is
    exactly zero in float64 (A = 0, beta = 0, reference row equal to the policy row but read through another stride) may
    carry the KL term's rounding: its allowance is then abs_err alone; a row whose allowance is zero must be exactly zero.

Reference rows, by (row index + kind) mod 4: equal to the policy row; the policy row plus N(0, 0.01); an independent draw of the
same kind (finite where the policy row holds -inf); the policy row plus N(0, 0.3) (the -inf rows: -inf exactly at the policy
row's -inf columns).  Row 17 (a -inf-off-the-label row) also gets -inf at some FINITE policy columns: outside the contract, so
it is left out of every gate and only shows that its neighbours are right."""
import math

import numpy as np
import pytest
import torch

from tests import policy_kl_ref as KR
from tests import policy_ref as PR
from tests import test_gpu_policy_edges as PE
from tests.test_gpu_policy_edges import BF, DEV, F32, NAN16, NAN32, U, bits, dev, dword, f64, sent16, sent32

pytestmark = pytest.mark.gpu
OUTSIDE = 17                                                         # the row outside the -inf contract
EQUAL, NEAR, INDEPENDENT, LOOSE = range(4)
KL_COEFS = (0.0, 0.05, 1.0)


def gate(name, ratios, limit):
    r = np.asarray(ratios, np.float64).reshape(-1)
    lim = np.broadcast_to(np.asarray(limit, np.float64), r.shape)
    if r.size == 0:
        return
    bad = ~(r <= lim)
    i = int(np.argmax(r))
    print(f"[policy-kl-edges] {name}: worst {r[i]:.3g} (gate {lim[i]:.3g})")
    assert not bad.any(), (name, int(np.argmax(bad)), float(r[np.argmax(bad)]), float(lim[np.argmax(bad)]))


def ref_rows(kinds, z, V, ld_ref, seed, outside=OUTSIDE):
    """the reference's logits [n, ld_ref] (NaN in columns V .. ld_ref: never read) and each row's kind"""
    rng = np.random.default_rng(seed + 1000)
    n = len(kinds)
    zr = np.full((n, ld_ref), np.nan, np.float32)
    fresh, _ = PE.pg_logits([k if k < PE.NEGINF_OFF else PE.NORMAL for k in kinds], V, V, seed + 2000)
    rk = np.array([(i + kinds[i]) % 4 for i in range(n)])
    for i in range(n):
        zi = z[i, :V]
        if rk[i] == EQUAL:
            zr[i, :V] = zi
        elif rk[i] == INDEPENDENT:
            zr[i, :V] = fresh[i]
        else:
            with np.errstate(invalid="ignore"):
                zr[i, :V] = zi + (rng.standard_normal(V) * (0.01 if rk[i] == NEAR else 0.3)).astype(np.float32)
    if outside is not None:
        fin = np.nonzero(np.isfinite(z[outside, :V]))[0]
        zr[outside, fin[::3][:5]] = -np.inf
    return zr, rk


def kl_allowances(fw, al, gs, kl_coef):
    """the docstring's E_KL and the gradient's abs_err with the KL term's share, from the float64 reference"""
    lse, rlse, p = fw["lse"], fw["ref_lse"], fw["p"]
    A, Ar = al["A"], U * (256 + 4 * np.abs(rlse))
    EKL = U * (512 + 6 * np.abs(lse) + 6 * np.abs(rlse) + 518 * fw["adiff"])
    with np.errstate(invalid="ignore"):
        el = np.where(p > 0, p * ((A + 4 * U)[:, None] * np.abs(fw["dk"] - fw["kl_raw"][:, None]) + (A + Ar + EKL)[:, None]), 0.0).max(1)
    return dict(Ar=Ar, EKL=EKL, abs_err=al["abs_err"] + abs(gs * kl_coef) * el * fw["has"])


def grad_ratio(got, ref, abs_err):
    """err / ((BF + F32) max|ref| + abs_err) per row; a row with a zero allowance must be exactly zero"""
    with np.errstate(invalid="ignore"):                             # (the row outside the -inf contract may hold NaN)
        err = np.abs(got - ref).max(1)
    allow = (BF + F32) * np.abs(ref).max(1) + abs_err
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), np.where(err == 0, 0.0, np.inf))


SHAPES = [(30522, 30528, 30528), (30522, 30522, 30528), (30522, 30528, 30522), (4100, 4100, 4100), (4096, 4096, 4097),
          (1000, 1001, 1000), (8, 8, 8), (3, 4, 3), (1, 1, 1)]


@pytest.mark.parametrize("V,ld,ld_ref", SHAPES)
def test_pg_kl_loss_numerical_edges(V, ld, ld_ref):
    from unimm_amd import lib
    kinds, z, y, adv, b = PE.build_rows(V, ld, seed=V + ld)
    n = len(y)
    zr, rk = ref_rows(kinds, z, V, ld_ref, seed=V + ld_ref)
    gated = np.arange(n) != OUTSIDE
    rng = np.random.default_rng(V)
    pos = rng.permutation(np.arange(n) * 3 + 1)
    adv_p, b_p = np.full(3 * n + 2, np.nan, np.float32), np.full(3 * n + 2, np.nan, np.float32)
    adv_p[pos], b_p[pos] = adv, b
    zg, zrg, yg = torch.from_numpy(z).to(DEV), torch.from_numpy(zr).to(DEV), dev(y, np.int32)
    g, inv = 0.75, 1.0 / 37
    gs = float(np.float32(g) * np.float32(inv))
    gdev = dword(g, torch.float32)
    ldd = (V + 7) // 8 * 8 + 8
    a64, b64 = adv.astype(np.float64), b.astype(np.float64)
    assert (kinds[OUTSIDE] == PE.NEGINF_OFF) and y[OUTSIDE] >= 0
    for ci, (mode, eps) in enumerate(((PR.LOGP, math.inf), (PR.RATIO, PE.EPS))):
        for beta in (0.0, 0.01):
            with_pos = bool((ci + (beta > 0)) % 2)
            pg = dev(pos, np.int32) if with_pos else None
            ag, bg = (dev(adv_p, np.float32), dev(b_p, np.float32)) if with_pos else (dev(adv, np.float32), dev(b, np.float32))
            if mode == PR.LOGP:
                bg = None
            # the existing pair on the same arguments: the bit-exact yardstick of property (1)
            o_loss, o_nll, o_lse, o_ent = sent32(n), sent32(n), sent32(n), sent32(n)
            lib.pg_loss_fwd(zg, yg, pg, ag, bg, mode, eps, beta, o_loss, o_nll, o_lse, o_ent, n, V)
            o_dl = sent16(n, ldd)
            lib.pg_loss_bwd(zg, yg, pg, ag, bg, mode, eps, beta, o_lse, o_ent, gdev, inv, o_dl, n, V)
            for kl_coef in KL_COEFS:
                tag = (f"V={V} ld={ld} ld_ref={ld_ref} mode={'ratio' if mode else 'logp'} beta={beta} kl_coef={kl_coef} "
                       f"pos={'given' if with_pos else 'NULL'}")
                fw = KR.forward(z[:, :V], zr[:, :V], y, adv, b, mode, eps, beta, kl_coef)
                grad_r = KR.backward(fw, y, beta, gs)[0]
                al = PE.allowances(fw, gs, beta, mode, a64, b64, y)
                ka = kl_allowances(fw, al, gs, kl_coef)
                A, EH, EKL = al["A"], al["EH"], ka["EKL"]
                rowloss, rownll, lse, ent, kl, rlse = (sent32(n) for _ in range(6))
                lib.pg_kl_loss_fwd(zg, yg, pg, ag, bg, mode, eps, beta, rowloss, rownll, lse, ent, n, V, zrg, kl_coef, kl, rlse)
                dl = sent16(n, ldd)
                lib.pg_kl_loss_bwd(zg, yg, pg, ag, bg, mode, eps, beta, lse, ent, gdev, inv, dl, n, V, zrg, kl_coef, kl, rlse)
                torch.cuda.synchronize()
                # (1) the non-KL outputs, and with kl_coef = 0 rowloss and dlogits, are the existing pair's bit for bit
                for name, mine, theirs in (("lse", lse, o_lse), ("ent", ent, o_ent), ("rownll", rownll, o_nll)):
                    assert (bits(mine) == bits(theirs)).all(), (tag, name, "differs from unimm_pg_loss_fwd")
                if kl_coef == 0.0:
                    assert (bits(rowloss)[gated] == bits(o_loss)[gated]).all(), (tag, "rowloss with kl_coef = 0")
                    assert (bits(dl) == bits(o_dl)).all(), (tag, "dlogits with kl_coef = 0")
                got = {k: f64(t) for k, t in (("lse", lse), ("ent", ent), ("rowloss", rowloss), ("rownll", rownll), ("kl", kl),
                                              ("ref_lse", rlse))}
                gd = f64(dl)
                for k, v in got.items():
                    assert not np.isnan(v[gated]).any(), (tag, k)             # no NaN in the gated rows, the -inf rows included
                assert not np.isnan(gd[gated]).any(), tag
                has = fw["has"]
                hg = has & gated
                gate(f"ref_lse {tag} (abs / A)", (np.abs(got["ref_lse"] - fw["ref_lse"]) / ka["Ar"])[gated], 1.0)
                cancels = EKL > 2.0 ** -10 * np.abs(fw["kl_raw"])
                with np.errstate(invalid="ignore"):                     # (the row outside the -inf contract may hold NaN)
                    kerr = np.abs(got["kl"] - fw["kl"]) / EKL
                gate(f"kl {tag} (abs / E_KL)", kerr[hg & ~cancels], 1.0)
                gate(f"kl {tag} (abs / E_KL, rows whose KL cancels)", kerr[hg & cancels], 1.0)
                assert (got["kl"][hg] >= -EKL[hg]).all()
                assert (bits(kl)[~has] == 0).all() and (got["rowloss"][~has] == 0).all() and (got["rownll"][~has] == 0).all()
                lfin = hg & np.isfinite(fw["rowloss"])
                assert (got["rowloss"][hg & ~lfin] == fw["rowloss"][hg & ~lfin]).all()
                a_abs = np.abs(a64)
                with np.errstate(invalid="ignore"):
                    loss_allow = ((a_abs * fw["r"] * al["rho"] if mode == PR.RATIO else a_abs * A) + beta * EH + kl_coef * EKL
                                  + 1e-6 * np.abs(fw["rowloss"]))
                gate(f"rowloss {tag} (abs)", np.abs(got["rowloss"][lfin] - fw["rowloss"][lfin]), loss_allow[lfin])
                ratio = grad_ratio(gd[:, :V], grad_r, ka["abs_err"])
                den = np.abs(grad_r).max(1)
                tight = ka["abs_err"] < F32 * den
                gate(f"grad {tag} (err / allowance)", ratio[gated & tight], 1.0)
                gate(f"grad {tag} (err / allowance, rows with a cancelling term)", ratio[gated & ~tight], 1.0)
                assert (bits(dl[:, V:]) == 0).all(), "dlogits columns V .. ldd must be zero"
                assert (bits(dl)[~has] == 0).all(), "an unlabelled row has an exactly zero gradient, whatever kl_coef is"
                assert (adv[~has] != 0).any()
                if kl_coef > 0 and beta == 0.0 and V >= 1000:
                    # A == 0 does not switch the KL term off (nor a clipped ratio): those rows' gradient is the KL term's
                    quiet = hg & ((adv == 0) | fw["clipped"]) & (rk != EQUAL)
                    assert quiet.sum() >= 3 and (np.abs(grad_r[quiet]).max(1) > 0).all() and (np.abs(gd[quiet]).max(1) > 0).all()
                inf_rows = ((kinds == PE.NEGINF_OFF) | (kinds == PE.NEGINF_ON)) & gated
                assert inf_rows.sum() == 7 and np.isfinite(gd[inf_rows]).all() and np.isfinite(got["kl"][inf_rows]).all()
                dead = np.isinf(z[:, :V]) & gated[:, None]                      # p_i = 0 off the label: an exactly zero element,
                dead[np.nonzero(has)[0], y[has]] = False                        # whatever the reference holds there
                assert (dead.sum() >= 7 or V < 8) and (gd[:, :V][dead] == 0).all()
            # (2) the reference IS the policy's buffer: KL = +0, ref_lse = lse bitwise, dlogits the existing pair's for any kl_coef
            for kl_coef in (0.05, 1.0):
                rowloss, rownll, lse, ent, kl, rlse = (sent32(n) for _ in range(6))
                lib.pg_kl_loss_fwd(zg, yg, pg, ag, bg, mode, eps, beta, rowloss, rownll, lse, ent, n, V, zg, kl_coef, kl, rlse)
                dl = sent16(n, ldd)
                lib.pg_kl_loss_bwd(zg, yg, pg, ag, bg, mode, eps, beta, lse, ent, gdev, inv, dl, n, V, zg, kl_coef, kl, rlse)
                torch.cuda.synchronize()
                assert (bits(kl) == 0).all(), "KL of a row against itself is exactly +0"
                assert (bits(rlse) == bits(lse)).all() and (bits(lse) == bits(o_lse)).all()
                assert (f64(rowloss) == f64(o_loss)).all() and (bits(dl) == bits(o_dl)).all()


CAP = 40


@pytest.mark.parametrize("count", [0, 1, CAP - 1, CAP, CAP + 7])
def test_pg_kl_loss_device_count(count):
    """n_dev / inv_dev: rows at or past the count are neither read (NaN logits in BOTH buffers, positions that point at NaN
    advantages) nor written (sentinels survive, kl and ref_lse included); inv_dev overrides the host float."""
    from unimm_amd import lib
    from oracle import rows_ref as RR
    V, ld, ld_ref, cap = 1000, 1004, 1001, CAP
    live = RR.live(count, cap)
    total = cap + 8
    rng = np.random.default_rng(count)
    z, y = PE.pg_logits([PE.NORMAL] * total, V, ld, seed=count)
    zr, _ = ref_rows([PE.NORMAL] * total, z, V, ld_ref, seed=count, outside=None)
    adv = rng.standard_normal(total).astype(np.float32)
    y[2::7] = -1
    base = PR.forward(z[:, :V], y, np.zeros(total), None, PR.LOGP, math.inf, 0.0)
    b = (base["logp"] - np.array([(-0.5, 0.0, 0.5)[i % 3] for i in range(total)])).astype(np.float32)
    pos = rng.permutation(np.arange(total) * 2)
    adv_p, b_p = np.full(2 * total, np.nan, np.float32), np.full(2 * total, np.nan, np.float32)
    adv_p[pos[:live]], b_p[pos[:live]] = adv[:live], b[:live]
    z[live:] = np.nan
    zr[live:] = np.nan
    mode, eps, beta, inv, kl_coef = PR.RATIO, PE.EPS, 0.01, 0.125, 0.5
    gs = 0.5 * inv
    zg, zrg, yg, pg = torch.from_numpy(z).to(DEV), torch.from_numpy(zr).to(DEV), dev(y, np.int32), dev(pos, np.int32)
    ag, bg = dev(adv_p, np.float32), dev(b_p, np.float32)
    n_dev, inv_dev, gdev = dword(count), dword(inv, torch.float32), dword(0.5, torch.float32)
    outs = [sent32(total) for _ in range(6)]
    rowloss, rownll, lse, ent, kl, rlse = outs
    lib.pg_kl_loss_fwd(zg, yg, pg, ag, bg, mode, eps, beta, rowloss, rownll, lse, ent, cap, V, zrg, kl_coef, kl, rlse, n_dev=n_dev)
    dl = sent16(total, 1008)
    lib.pg_kl_loss_bwd(zg, yg, pg, ag, bg, mode, eps, beta, lse, ent, gdev, 99.0, dl, cap, V, zrg, kl_coef, kl, rlse, n_dev=n_dev,
                       inv_dev=inv_dev)
    torch.cuda.synchronize()
    for name, t in zip(("rowloss", "rownll", "lse", "ent", "kl", "ref_lse"), outs):
        assert (bits(t[live:]) == NAN32).all(), f"pg_kl_loss_fwd {name}: rows past the count are not written"
    assert (bits(dl[live:]) == np.int16(NAN16)).all(), "pg_kl_loss_bwd: rows past the count are not written"
    if live:
        fw = KR.forward(z[:live, :V], zr[:live, :V], y[:live], adv[:live], b[:live], mode, eps, beta, kl_coef)
        grad_r = KR.backward(fw, y[:live], beta, gs)[0]
        al = PE.allowances(fw, gs, beta, mode, adv[:live].astype(np.float64), b[:live].astype(np.float64), y[:live])
        ka = kl_allowances(fw, al, gs, kl_coef)
        gate("(n_dev) lse (abs / A)", np.abs(f64(lse[:live]) - fw["lse"]) / al["A"], 1.0)
        gate("(n_dev) ref_lse (abs / A)", np.abs(f64(rlse[:live]) - fw["ref_lse"]) / ka["Ar"], 1.0)
        gate("(n_dev) kl (abs / E_KL)", np.abs(f64(kl[:live]) - fw["kl"]) / ka["EKL"], 1.0)
        gate("(n_dev) rowloss (abs)", np.abs(f64(rowloss[:live]) - fw["rowloss"]),
             np.abs(adv[:live]) * fw["r"] * al["rho"] + beta * al["EH"] + kl_coef * ka["EKL"] + 1e-6 * np.abs(fw["rowloss"]))
        gate("(n_dev, inv_dev) grad (err / allowance)", grad_ratio(f64(dl[:live, :V]), grad_r, ka["abs_err"]), 1.0)
        assert (bits(dl[:live, V:]) == 0).all()
        assert np.isnan(f64(zg)).any() and not np.isnan(f64(dl[:live])).any()


def test_pg_kl_loss_refused_arguments():
    from unimm_amd import lib
    z = torch.zeros((2, 8), device=DEV)
    y = torch.zeros(2, dtype=torch.int32, device=DEV)
    adv = torch.zeros(2, device=DEV)
    o = [torch.zeros(2, device=DEV) for _ in range(4)]
    kl, rlse, g = torch.zeros(2, device=DEV), torch.zeros(2, device=DEV), torch.ones(1, device=DEV)
    dl = torch.zeros((2, 8), dtype=torch.bfloat16, device=DEV)

    def fwd(ref=z, kl_coef=0.1, kl=kl, rlse=rlse, mode=lib.PG_LOGP, a=adv):
        lib.pg_kl_loss_fwd(z, y, None, a, None, mode, 0.2, 0.0, *o, 2, 8, ref, kl_coef, kl, rlse)

    def bwd(ref=z, kl_coef=0.1, kl=kl, rlse=rlse, mode=lib.PG_LOGP, a=adv):
        lib.pg_kl_loss_bwd(z, y, None, a, None, mode, 0.2, 0.0, o[2], o[3], g, 1.0, dl, 2, 8, ref, kl_coef, kl, rlse)

    fwd(), bwd()                                                      # the accepted form
    refused = [dict(ref=None), dict(ref=torch.zeros((2, 7), device=DEV)), dict(kl_coef=-0.1), dict(kl_coef=math.inf),
               dict(kl_coef=math.nan), dict(kl=None), dict(rlse=None),
               dict(mode=lib.PG_RATIO), dict(mode=2), dict(a=adv[:1])]     # ... and the existing pair's refusals
    for kw in refused:
        for call in (fwd, bwd):
            with pytest.raises(lib.UnimmHipError):
                call(**kw)
    torch.cuda.synchronize()
