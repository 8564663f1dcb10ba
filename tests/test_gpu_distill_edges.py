"""unimm_distill_loss_fwd / unimm_distill_loss_bwd per element against the float64 restatement (tests/distill_ref.py), on the rows
of tests/test_gpu_policy_edges.py (normal, one dominant logit, huge magnitudes, flat, -inf off and on the label; every kind with
the weights 1, 3, -1 and 0) with the four kinds of teacher rows of tests/test_gpu_policy_kl_edges.py (equal, near, independent,
loose; rows, helpers and gates imported unchanged), at every (V, ld, ld_ref) at which the kernels take another path -- the
4096-float unrolled step, its remainders, the scalar tail, a vector student row beside a scalar teacher row and the reverse --
and at every edge a device-side row count can sit on.  Every gate is per row and printed next to its worst ratio.

The -inf contract is the KL pair's mirrored: the teacher rows get -inf wherever the student row holds it (q_i = 0 meets p_i = 0),
some teacher rows get -inf at FINITE student columns as well (q_i = 0 whatever z_i holds), and row 17 gets finite teacher logits
at some of the student's -inf columns: outside the contract (KD = +inf), left out of every gate; it only shows that its
neighbours are right.

Error budgets (U = 2^-24; every quantity is the float64 reference's, none is read from the kernel; tests/distill_ref.py's
`allowances` states them in code and tests/test_distill_cpu.py holds the CPU fp32 restatement of the forward inside them):

  * lse: tests/test_gpu_row_edges.py's A(x) = U (256 + 4 |x|).
  * lse_t = m / tau + log st and ref_lse_t: A's 256 roundings of the sum and 4 |x|, plus the roundings of the 1 / tau product.  An
    exponent (z_i - m) (1 / tau) carries three relative roundings (the subtraction, 1 / tau itself, the product), so a term of st
    is off by 3 U x_i relative, x_i = (m - z_i) / tau, and log st by 3 U sum_i p_i x_i <= 3 U log V (sum p x = H(p) - (lse_t -
    m / tau) <= log V).  m (1 / tau) + log st is one fma: 1 / tau's rounding and the fma's, 2 U |m / tau| <= 2 U (|x| + log V).
    With log V <= log 65536 = 11.1 that is 5 * 11.1 < 64 more roundings and 2 |x|:
        A_t(x) = U (320 + 6 |x|)   absolute.
  * KD = ur / (sr tau) - ref_lse_t + lse_t with ur = sum e^((zr_i - mr) / tau) (zr_i - z_i) accumulated beside sr, in its order.
    The KL pair budgets 258 roundings per term of its u and 256 for s; here a term's exponential also carries 3 U x_i relative,
    and a term that is not exactly 0 in fp32 has x_i < 104 (e^-104 < 2^-149): |dur| <= (258 + 312) U sum e |zr - z|, |dsr| <=
    (256 + 3 log V) U sr <= 290 U sr, so ur / (sr tau) = sum q_i (zr_i - z_i) / tau is off by (570 + 290 + 2) U sum q |zr - z| / tau
    (the + 2: the product sr tau and the division).  The two final subtractions round once each, on numbers of size <= sum
    q |zr - z| / tau + |ref_lse_t| (+ |lse_t|).  With A_t(lse_t) + A_t(ref_lse_t) that adds up to U (640 + 7 |lse_t| + 8 |ref_lse_t|
    + 864 sum q |zr - z| / tau), inside
        E_KD = U (640 + 8 |lse_t| + 8 |ref_lse_t| + 864 sum_i q_i |zr_i - z_i| / tau)   absolute
    (the KL pair's 6 and 518 plus the scaled products: a = 8, c = 864).  Rows where E_KD > 2^-10 |KD| (the two rows nearly agree)
    are gated by the same E_KD but reported apart.
  * rowloss: alpha (that file's allowance of the hard term: w A, the unlikelihood's cancellation bound) + (1 - alpha) tau^2 E_KD
    + 1e-6 |rowloss|.
  * the gradient: the KL file's gate, err <= (BF + F32) max|ref| + abs_err, with abs_err = the hard term's (|gs alpha c| (2 (A max p
    + 2 U) + the unlikelihood's 2 canc max|p - onehot|)) plus the soft term's share: p_i = e^(z_i (1 / tau) - lse_t) is one fma and
    one exponential, off by A_t(lse_t) + U (|log p_i| + |z_i| / tau + 4) relative, q_i likewise:
        |gs (1 - alpha) tau| max_i (p_i (A_t(lse_t) + U (|log p_i| + |z_i| / tau + 4)) + q_i (A_t(ref_lse_t) + U (|log q_i| + |zr_i| / tau + 4))).
    A row whose allowance is zero must be exactly zero.

Bit-exact properties (include/unimm_hip.h): (1) rownll and lse are unimm_lm_loss_fwd's wherever that kernel defines them (it
returns NaN for a row with -inf logits in a lane's first columns), and unimm_pg_loss_fwd's on every row; (2) alpha == 1: rowloss
and dlogits are unimm_lm_loss_fwd / _bwd's and the teacher's buffer, full of NaN, is not read; (3) the teacher IS the student's
buffer: kd = +0, ref_lse_t == lse_t, and with alpha == 0 an all-zero gradient; (4) tau == 1: lse_t == lse."""
import math

import numpy as np
import pytest
import torch

from tests import distill_ref as DR
from tests import test_gpu_policy_edges as PE
from tests import test_gpu_policy_kl_edges as KE
from tests.test_gpu_policy_edges import DEV, F32, NAN16, NAN32, bits, dev, dword, f64, sent16, sent32
from tests.test_gpu_policy_kl_edges import EQUAL, grad_ratio

pytestmark = pytest.mark.gpu
OUTSIDE = 17                                                         # the row outside the -inf contract
WEIGHTS = (1, 3, -1, 0)
TAUS = (1.0, 2.0, 0.5)
ALPHAS = (0.0, 0.5, 1.0)
SHAPES = KE.SHAPES


def gate(name, ratios, limit):
    r = np.asarray(ratios, np.float64).reshape(-1)
    lim = np.broadcast_to(np.asarray(limit, np.float64), r.shape)
    if r.size == 0:
        return
    bad = ~(r <= lim)
    i = int(np.argmax(r))
    print(f"[distill-edges] {name}: worst {r[i]:.3g} (gate {lim[i]:.3g})")
    assert not bad.any(), (name, int(np.argmax(bad)), float(r[np.argmax(bad)]), float(lim[np.argmax(bad)]))


def teacher_rows(kinds, z, V, ld_ref, seed, outside=OUTSIDE):
    """the teacher's logits [n, ld_ref] (NaN in columns V .. ld_ref: never read) and each row's kind: the KL file's reference
    rows, brought inside THIS pair's -inf contract (module docstring)"""
    zr, rk = KE.ref_rows(kinds, z, V, ld_ref, seed, outside=None)
    n = len(kinds)
    sinf = np.isinf(z[:, :V])
    zr[:, :V][sinf] = -np.inf
    for i in range(n):
        if rk[i] != EQUAL and i % 4 in (0, 1) and i != outside:      # q_i = 0 at finite student columns
            fin = np.nonzero(~sinf[i])[0]
            zr[i, fin[1::5][:7]] = -np.inf
    if outside is not None:
        cols = np.nonzero(sinf[outside])[0][:3]
        zr[outside, cols] = 0.5
    return zr, rk


def rows(V, ld, ld_ref):
    kinds, z, y, _, _ = PE.build_rows(V, ld, seed=V + ld)
    w = np.array([WEIGHTS[i % 4] for i in range(len(y))])
    zr, rk = teacher_rows(kinds, z, V, ld_ref, seed=V + ld_ref)
    return kinds, z, zr, y, w, rk


def run(lib, zg, yg, wg, zrg, tau, alpha, n, V, ldd, gdev, inv):
    out = [sent32(n) for _ in range(6)]
    rowloss, rownll, lse, lse_t, rlse_t, kd = out
    lib.distill_loss_fwd(zg, yg, wg, zrg, tau, alpha, rowloss, rownll, lse, lse_t, rlse_t, kd, n, V)
    dl = sent16(n, ldd)
    lib.distill_loss_bwd(zg, yg, wg, zrg, tau, alpha, lse, lse_t, rlse_t, gdev, inv, dl, n, V)
    torch.cuda.synchronize()
    return dict(rowloss=rowloss, rownll=rownll, lse=lse, lse_t=lse_t, ref_lse_t=rlse_t, kd=kd), dl


@pytest.mark.parametrize("V,ld,ld_ref", SHAPES)
def test_distill_loss_numerical_edges(V, ld, ld_ref):
    from unimm_amd import lib
    kinds, z, zr, y, w, rk = rows(V, ld, ld_ref)
    n = len(y)
    gated = np.arange(n) != OUTSIDE
    assert kinds[OUTSIDE] == PE.NEGINF_OFF and y[OUTSIDE] >= 0
    zg, zrg, yg, wg = torch.from_numpy(z).to(DEV), torch.from_numpy(zr).to(DEV), dev(y, np.int32), dev(w, np.int32)
    nan_teacher = torch.full_like(zrg, float("nan"))
    g, inv = 0.75, 1.0 / 37
    gs = float(np.float32(g) * np.float32(inv))
    gdev = dword(g, torch.float32)
    ldd = (V + 7) // 8 * 8 + 8
    # the yardsticks of properties (1) and (2): the likelihood pair and the policy-gradient forward on the same rows
    o_loss, o_nll, o_lse = sent32(n), sent32(n), sent32(n)
    lib.lm_loss_fwd(zg, yg, wg, o_loss, o_nll, o_lse, n, V)
    p_out = [sent32(n) for _ in range(4)]
    lib.pg_loss_fwd(zg, yg, None, torch.zeros(n, device=DEV), None, lib.PG_LOGP, math.inf, 0.0, *p_out, n, V)
    torch.cuda.synchronize()
    defined = ~np.isnan(f64(o_lse))                                   # the rows unimm_lm_loss_fwd defines
    assert defined[kinds < PE.NEGINF_OFF].all()
    for tau in TAUS:
        for alpha in ALPHAS:
            tag = f"V={V} ld={ld} ld_ref={ld_ref} tau={tau} alpha={alpha}"
            fw = DR.forward(z[:, :V], zr[:, :V], y, w, tau, alpha)
            grad_r = DR.backward(fw, y, w, gs)[0]
            al = DR.allowances(fw, z[:, :V], zr[:, :V], y, w, gs)
            out, dl = run(lib, zg, yg, wg, nan_teacher if alpha == 1.0 else zrg, tau, alpha, n, V, ldd, gdev, inv)
            got = {k: f64(t) for k, t in out.items()}
            gd = f64(dl)
            has, part = fw["has"], fw["part"]
            # (1) lse and rownll bit for bit
            for name, theirs in (("lse", o_lse), ("rownll", o_nll)):
                assert (bits(out[name])[defined] == bits(theirs)[defined]).all(), (tag, name, "differs from unimm_lm_loss_fwd")
            assert (bits(out["lse"]) == bits(p_out[2])).all() and (bits(out["rownll"]) == bits(p_out[1])).all(), (tag, "unimm_pg_loss_fwd")
            # (4) tau == 1: lse_t is lse
            if tau == 1.0:
                assert (bits(out["lse_t"]) == bits(out["lse"])).all(), (tag, "lse_t != lse at tau = 1")
            # (2) alpha == 1: the likelihood pair's bits, the teacher (NaN everywhere) not read
            if alpha == 1.0:
                assert (bits(out["rowloss"])[defined] == bits(o_loss)[defined]).all(), (tag, "rowloss with alpha = 1")
                assert (bits(out["kd"]) == 0).all() and (bits(out["ref_lse_t"]) == 0).all()
                o_dl = sent16(n, ldd)
                lib.lm_loss_bwd(zg, yg, wg, out["lse"], gdev, inv, o_dl, n, V)
                torch.cuda.synchronize()
                zc = al["zero_coef"]
                assert (bits(dl)[~zc] == bits(o_dl)[~zc]).all(), (tag, "dlogits with alpha = 1")
                assert (bits(dl)[zc] == 0).all() and (f64(o_dl)[zc] == 0).all() and zc.sum() >= 6 and (~zc).sum() >= 12
            for k, v in got.items():
                assert not np.isnan(v[gated]).any(), (tag, k)         # no NaN in the gated rows, the -inf rows included
            assert not np.isnan(gd[gated]).any(), tag
            gate(f"lse {tag} (abs / A)", (np.abs(got["lse"] - fw["lse"]) / al["A"])[gated], 1.0)
            gate(f"lse_t {tag} (abs / A_t)", (np.abs(got["lse_t"] - fw["lse_t"]) / al["At"])[gated], 1.0)
            fin = has & np.isfinite(fw["rownll"]) & gated
            gate(f"rownll {tag} (abs)", np.abs(got["rownll"] - fw["rownll"])[fin], (al["A"] + 1e-6 * np.abs(fw["rownll"]))[fin])
            assert (got["rownll"][has & ~fin & gated] == np.inf).all() and (got["rownll"][~has] == 0).all()
            pg = part & gated
            if alpha != 1.0:
                gate(f"ref_lse_t {tag} (abs / A_t)", (np.abs(got["ref_lse_t"] - fw["ref_lse_t"]) / al["Art"])[gated], 1.0)
                EKD = al["EKD"]
                cancels = EKD > 2.0 ** -10 * np.abs(fw["kd_raw"])
                with np.errstate(invalid="ignore"):                   # (the row outside the -inf contract holds inf)
                    kerr = np.abs(got["kd"] - fw["kd"]) / EKD
                gate(f"kd {tag} (abs / E_KD)", kerr[pg & ~cancels], 1.0)
                gate(f"kd {tag} (abs / E_KD, rows whose KD cancels)", kerr[pg & cancels], 1.0)
                assert (got["kd"][pg] >= -EKD[pg]).all()
                assert (pg & ~cancels).sum() >= 3 or V < 1000
            assert (bits(out["kd"])[~part] == 0).all() and (bits(out["rowloss"])[~part] == 0).all()
            lfin = pg & np.isfinite(fw["rowloss"])
            assert (got["rowloss"][pg & ~lfin] == fw["rowloss"][pg & ~lfin]).all()       # +inf: -inf on the label, alpha > 0
            gate(f"rowloss {tag} (abs)", np.abs(got["rowloss"] - fw["rowloss"])[lfin], al["loss"][lfin])
            ratio = grad_ratio(gd[:, :V], grad_r, al["abs_err"])
            den = np.abs(grad_r).max(1)
            tight = al["abs_err"] < F32 * den
            gate(f"grad {tag} (err / allowance)", ratio[gated & tight], 1.0)
            gate(f"grad {tag} (err / allowance, rows with a cancelling term)", ratio[gated & ~tight], 1.0)
            assert (bits(dl[:, V:]) == 0).all(), "dlogits columns V .. ldd must be zero"
            assert (bits(dl)[~part] == 0).all(), "a row with y < 0 or w == 0 has an exactly zero gradient"
            assert (~has).sum() == 3 and (has & (w == 0)).sum() >= 4
            inf_rows = ((kinds == PE.NEGINF_OFF) | (kinds == PE.NEGINF_ON)) & gated
            assert inf_rows.sum() == 7 and np.isfinite(gd[inf_rows]).all() and np.isfinite(got["kd"][inf_rows]).all()
            if alpha != 1.0 and V >= 8:
                dead = np.isinf(zr[:, :V]) & np.isfinite(z[:, :V]) & pg[:, None]     # q_i = 0 at a finite z_i: the element is
                assert dead.sum() >= 7                                               # the student's own share
            if alpha == 0.0 and V >= 1000:                            # the soft term alone moves a row that takes part
                moving = pg & (rk != EQUAL) & ((kinds == PE.NORMAL) | (kinds == PE.FLAT))
                assert moving.sum() >= 3 and (np.abs(grad_r[moving]).max(1) > 0).all() and (np.abs(gd[moving]).max(1) > 0).all()
        # (3) the teacher IS the student's buffer: kd = +0, ref_lse_t = lse_t bitwise, a soft term of exactly zero
        for alpha in (0.0, 0.5):
            out, dl = run(lib, zg, yg, wg, zg, tau, alpha, n, V, ldd, gdev, inv)
            assert (bits(out["kd"]) == 0).all(), "KD of a row against itself is exactly +0"
            assert (bits(out["ref_lse_t"]) == bits(out["lse_t"])).all()
            if alpha == 0.0:
                assert (bits(dl) == 0).all() and (bits(out["rowloss"]) == 0).all()
            else:                                                     # ... and what is left is the hard term's share
                fw = DR.forward(z[:, :V], z[:, :V], y, w, tau, alpha)
                al = DR.allowances(fw, z[:, :V], z[:, :V], y, w, gs)
                hard = DR.backward(fw, y, w, gs)[1]
                gate(f"grad V={V} tau={tau} alpha={alpha}, teacher == student (err / the hard term's allowance)",
                     grad_ratio(f64(dl)[:, :V], hard, al["abs_err"]), 1.0)


CAP = 40


@pytest.mark.parametrize("count", [0, 1, CAP - 1, CAP, CAP + 7])
def test_distill_loss_device_count(count):
    """n_dev / inv_dev: rows at or past the count are neither read (NaN logits in BOTH buffers) nor written (sentinels survive,
    lse_t, ref_lse_t and kd included); inv_dev overrides the host float."""
    from unimm_amd import lib
    from oracle import rows_ref as RR
    V, ld, ld_ref, cap = 1000, 1004, 1001, CAP
    live = RR.live(count, cap)
    total = cap + 8
    z, y = PE.pg_logits([PE.NORMAL] * total, V, ld, seed=count)
    zr, _ = KE.ref_rows([PE.NORMAL] * total, z, V, ld_ref, seed=count, outside=None)
    w = np.array([WEIGHTS[i % 4] for i in range(total)])
    y[2::7] = -1
    z[live:] = np.nan
    zr[live:] = np.nan
    tau, alpha, inv = 2.0, 0.5, 0.125
    gs = 0.5 * inv
    zg, zrg, yg, wg = torch.from_numpy(z).to(DEV), torch.from_numpy(zr).to(DEV), dev(y, np.int32), dev(w, np.int32)
    n_dev, inv_dev, gdev = dword(count), dword(inv, torch.float32), dword(0.5, torch.float32)
    outs = [sent32(total) for _ in range(6)]
    rowloss, rownll, lse, lse_t, rlse_t, kd = outs
    lib.distill_loss_fwd(zg, yg, wg, zrg, tau, alpha, rowloss, rownll, lse, lse_t, rlse_t, kd, cap, V, n_dev=n_dev)
    dl = sent16(total, 1008)
    lib.distill_loss_bwd(zg, yg, wg, zrg, tau, alpha, lse, lse_t, rlse_t, gdev, 99.0, dl, cap, V, n_dev=n_dev, inv_dev=inv_dev)
    torch.cuda.synchronize()
    for name, t in zip(("rowloss", "rownll", "lse", "lse_t", "ref_lse_t", "kd"), outs):
        assert (bits(t[live:]) == NAN32).all(), f"distill_loss_fwd {name}: rows past the count are not written"
    assert (bits(dl[live:]) == np.int16(NAN16)).all(), "distill_loss_bwd: rows past the count are not written"
    if live:
        fw = DR.forward(z[:live, :V], zr[:live, :V], y[:live], w[:live], tau, alpha)
        grad_r = DR.backward(fw, y[:live], w[:live], gs)[0]
        al = DR.allowances(fw, z[:live, :V], zr[:live, :V], y[:live], w[:live], gs)
        gate("(n_dev) lse (abs / A)", np.abs(f64(lse[:live]) - fw["lse"]) / al["A"], 1.0)
        gate("(n_dev) lse_t (abs / A_t)", np.abs(f64(lse_t[:live]) - fw["lse_t"]) / al["At"], 1.0)
        gate("(n_dev) ref_lse_t (abs / A_t)", np.abs(f64(rlse_t[:live]) - fw["ref_lse_t"]) / al["Art"], 1.0)
        gate("(n_dev) kd (abs / E_KD)", np.abs(f64(kd[:live]) - fw["kd"]) / al["EKD"], 1.0)
        gate("(n_dev) rowloss (abs)", np.abs(f64(rowloss[:live]) - fw["rowloss"]), al["loss"])
        gate("(n_dev, inv_dev) grad (err / allowance)", grad_ratio(f64(dl[:live, :V]), grad_r, al["abs_err"]), 1.0)
        assert (bits(dl[:live, V:]) == 0).all()
        assert np.isnan(f64(zg)).any() and not np.isnan(f64(dl[:live])).any()


def test_distill_loss_refused_arguments():
    from unimm_amd import lib
    z = torch.zeros((2, 8), device=DEV)
    y = torch.zeros(2, dtype=torch.int32, device=DEV)
    w = torch.ones(2, dtype=torch.int32, device=DEV)
    o = [torch.zeros(2, device=DEV) for _ in range(6)]
    g = torch.ones(1, device=DEV)
    dl = torch.zeros((2, 8), dtype=torch.bfloat16, device=DEV)

    def fwd(ref=z, tau=2.0, alpha=0.5, z=z, y=y, w=w, o=o, V=8):
        lib.distill_loss_fwd(z, y, w, ref, tau, alpha, *o, 2, V)

    def bwd(ref=z, tau=2.0, alpha=0.5, z=z, y=y, w=w, o=o, V=8):
        lib.distill_loss_bwd(z, y, w, ref, tau, alpha, o[2], o[3], o[4], g, 1.0, dl, 2, V)

    fwd(), bwd()                                                      # the accepted forms
    fwd(ref=None, alpha=1.0), bwd(ref=None, alpha=1.0)                # alpha == 1 needs no teacher
    refused = [dict(ref=None), dict(ref=torch.zeros((2, 7), device=DEV)), dict(tau=0.0), dict(tau=-1.0), dict(tau=math.inf),
               dict(tau=math.nan), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=math.nan), dict(y=None), dict(w=None),
               dict(o=[None] + o[1:]), dict(o=o[:3] + [None] + o[4:]), dict(o=o[:4] + [None] + o[5:]),
               dict(V=0), dict(V=9)]                                  # ... and the likelihood pair's shapes
    for kw in refused:
        for call in (fwd, bwd):
            if call is bwd and kw.get("o") is not None and kw["o"][0] is None:
                continue                                              # (rowloss: the forward's alone)
            with pytest.raises(lib.UnimmHipError):
                call(**kw)
    with pytest.raises(lib.UnimmHipError):
        lib.distill_loss_fwd(z, y, w, z, 2.0, 0.5, *o[:5], None, 2, 8)    # kd
    with pytest.raises(lib.UnimmHipError):
        lib.distill_loss_bwd(z, y, w, z, 2.0, 0.5, o[2], o[3], o[4], g, 1.0, torch.zeros((2, 12), dtype=torch.bfloat16, device=DEV), 2, 8)
    torch.cuda.synchronize()
