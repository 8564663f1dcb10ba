"""unimm_lm_spec_verify restated for the tests (TEST INFRASTRUCTURE, the rule of tests/sample_ref.py): the float64 restatement of
one launch built on sample_ref.Row / sample_row, the host mirror of the accept uniform, a float32 restatement in the kernel's
order of operations that the constants were measured with, and the cases.

Semantics (include/unimm_hip.h): P~ / Q~ = the sampler's filtered distributions of the rows x / xd under the same banned ids,
flags and (temperature, top_k, top_p); a = log P~_d - log Q~_d (+inf: d not in K_Q, -inf: d not in K_P); accept iff log u < a;
on reject token = argmax over {i in K_P, rho_i < 1} of y_i + log1p(-rho_i) + g_i, rho = Q~ / P~ (0 outside K_Q), no candidate:
the first id of P~'s rank order; logq = log P~_token, logp = x_token - lse.

Budgets (u = 2^-24; form_R(i) = 1 + ln |K_R| + |lse_y| + |log R~_i| is sample_ref's E_logq / (C_Q u) on row R):
  accept   DECIDED when |log u - a| > E_acc = C_ACC u (form_P(d) + form_Q(d) + |log u| + |a|): the two log-probabilities with
           E_logq's form each, the rounding of logf(u) and of the difference.  A decided accept must be the float64 one.
  log rho  delta_i = E_logq^P(i) + E_logq^Q(i) (sample_ref's own budgets, C_Q): whether rho_i < 1 is CERTAIN only when
           |log rho_i| > delta_i.
  residual id i's perturbed value carries E_i = C_RES u ((1 + max |y| + max |g| + |log1p(-rho_i)|) + rho_i / (1 - rho_i)
           (form_P(i) + form_Q(i))): E_draw's form plus the conditioning of log1p(-rho) on the error of log rho.  With
           lo_i = w_i - E_i (-inf when i may stop being a candidate) and hi_i = w_i + E_i (for an id whose float64 rho is >= 1 but
           not certainly: y_i + g_i + log1p(-exp(log rho_i - delta_i)) + E_i) the ADMISSIBLE tokens are {i : hi_i >= max lo};
           the draw is DECIDED when that is one id (the float64 gap between the best and every other value exceeds both budgets).
  nucleus  sample_ref's membership exemptions apply to both rows: every pair of admissible kept-set sizes (K_P, K_Q) is a
           reading of the row, and the kernel's outputs must satisfy one of them.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from tests import sample_ref as SR

U32 = SR.U32
SEP = SR.SEP

# measured on the CPU over spec_case(V), V in SPEC_V, the three launches of `launch_params` each
# (tests/test_spec_sample_cpu.py::test_f32_restatement_inside_budgets prints them again):
ACC_MEASURED = 0.439      # worst |fp32 (a - log u) - fp64| / (u (form_P(d) + form_Q(d) + |log u| + |a|))
C_ACC = 4.0               # the power of two >= 8 x ACC_MEASURED
RES_MEASURED = 2.541      # worst |fp32 perturbed residual value - fp64| / (E_i / C_RES)
C_RES = 32.0              # the power of two >= 8 x RES_MEASURED

KEY_ACCEPT = 0x0ACCE97A
KEY_RESIDUAL = 0x5E51D0A1
KEY_DRAFT = 0x0D4AF7ED
SPEC_V = (16, 257, 30522, 65536)
TEMPS = (1.0, 0.7, 2.0)
TOP_KS = (0, 1, 2, 50)
TOP_PS = (1.0, 0.9, 1e-6)
ROWS = 64
UNDECIDED_CAP = 0.02


def accept_uniform(key, stream):
    """u of step 7: the sampler's u_0 of (key_accept, stream) -> float (exact in float32)."""
    return float(SR.uniforms(key, stream, np.zeros(1, dtype=np.int64))[0])


# ---------------------------------------------------------------------------------------------------------------------------
# one row, float64
# ---------------------------------------------------------------------------------------------------------------------------
def kept_sets(row, temperature, top_k, top_p):
    """The admissible kept sets of a sample_ref.Row -> list of dict(L, ids, y (absolute x / t), logr (log R~), form, E) -- the
    first is the float64 one; [] when nothing is eligible."""
    ref = SR.sample_row(row, temperature, top_k, top_p)
    if ref["n"] == 0:
        return []
    t = float(np.float32(temperature))
    out = []
    for L in ref["lengths"]:
        y = row.x[:L] / t
        lse_y = y[0] + math.log(float(np.exp(y - y[0]).sum()))
        logr = y - lse_y
        form = 1.0 + math.log(L) + abs(lse_y) + np.abs(logr)
        out.append(dict(L=L, ids=row.ids[:L], y=y, logr=logr, form=form, E=SR.C_Q * U32 * form, g=row.g[:L]))
    return out


def _lookup(kq, V):
    """id -> (log Q~, form) as dense arrays (-inf / 0 outside K_Q)."""
    lq, fq = np.full(V, -np.inf), np.zeros(V)
    if kq is not None:
        lq[kq["ids"]] = kq["logr"]
        fq[kq["ids"]] = kq["form"]
    return lq, fq


def verify_reading(kp, kq, d, V, u):
    """One reading (K_P, K_Q) of a row -> dict(a, accept, acc_decided, E_acc, allowed {id}, res_decided, res_token, first)."""
    lq, fq = _lookup(kq, V)
    pos = {int(i): n for n, i in enumerate(kp["ids"])} if 0 <= d < V else {}
    a, E_acc = -math.inf, 0.0
    logu = math.log(u)
    if d in pos:
        n = pos[d]
        if lq[d] > -np.inf:
            a = float(kp["logr"][n] - lq[d])
            E_acc = C_ACC * U32 * (float(kp["form"][n]) + float(fq[d]) + abs(logu) + abs(a))
        else:
            a = math.inf
    accept = logu < a
    acc_decided = math.isinf(a) or abs(logu - a) > E_acc
    # the residual
    ids, y, g = kp["ids"], kp["y"], kp["g"]
    lr = lq[ids] - kp["logr"]                                           # log rho (-inf: rho = 0)
    delta = SR.C_Q * U32 * (kp["form"] + fq[ids])
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        rho = np.exp(lr)
        cand = rho < 1.0
        l1 = np.where(cand, np.log1p(-np.where(cand, rho, 0.0)), -np.inf)
        w = y + l1 + g
        cond = np.where(cand, rho / np.where(cand, 1.0 - rho, 1.0), 0.0)
        E = C_RES * U32 * ((1.0 + np.abs(y).max() + np.abs(g).max() + np.where(cand, np.abs(l1), 0.0)) + cond * (kp["form"] + fq[ids]))
        certain = cand & ((lr + delta < 0.0) | (lr == -np.inf))
        maybe = ~cand & (lr - delta < 0.0)                              # float64 says rho >= 1, float32 may say < 1
        hi = np.where(cand, w + E, -np.inf)
        l1_hi = np.log1p(-np.exp(np.where(maybe, lr - delta, -1.0)))
        hi = np.where(maybe, y + g + l1_hi + E, hi)
        lo = np.where(certain, w - E, -np.inf)
    first = int(ids[0])
    level = float(lo.max())
    allowed = {int(i) for i in ids[(hi >= level) & (hi > -np.inf)]}
    if not np.isfinite(level):
        allowed.add(first)                                              # every candidate may vanish: the fallback
    res_token = first
    if cand.any():
        best = np.nonzero(w == w[cand].max())[0]
        best = best[cand[best]]
        res_token = int(ids[best[np.argmin(ids[best])]])
    return dict(a=a, accept=bool(accept), acc_decided=bool(acc_decided), E_acc=E_acc, allowed=allowed,
                res_decided=len(allowed) == 1, res_token=res_token, first=first, logu=logu)


def verify_row(rowp, rowq, d, temperature, top_k, top_p, key_accept, V):
    """float64 restatement of one row -> list of readings (the first: the float64 kept sets), [] when x has nothing eligible."""
    kps = kept_sets(rowp, temperature, top_k, top_p)
    kqs = (kept_sets(rowq, temperature, top_k, top_p) if d != -1 else []) or [None]
    u = accept_uniform(key_accept, rowp.stream)
    return [dict(verify_reading(kp, kq, d, V, u), kp=kp) for kp in kps for kq in kqs]


def row_decided(readings, d):
    """Whether the reference alone fixes (accept, token): every reading decides both, and all readings agree."""
    outcomes = set()
    for rd in readings:
        if not rd["acc_decided"] or (not rd["accept"] and not rd["res_decided"]):
            return False
        outcomes.add((True, d) if rd["accept"] else (False, next(iter(rd["allowed"]))))
    return len(outcomes) == 1


def bad_params(t, k, p):
    t, p = float(np.float32(t)), float(np.float32(p))
    return not (t > 0.0 and t < math.inf and 0.0 < p <= 1.0 and k >= 0)


def check_launch(rowsp, rowsq, draft, params, key_accept, V, out, what=""):
    """out: dict of host arrays accept, token, logp, logq, lse, log_ratio -> (rows with a draw, undecided rows)."""
    from oracle import generate_ref as GR
    draws = undecided = 0
    for r, (rp, rq) in enumerate(zip(rowsp, rowsq)):
        t, k, p = float(params[0][r]), int(params[1][r]), float(params[2][r])
        d, tk, acc = int(draft[r]), int(out["token"][r]), int(out["accept"][r])
        lse64 = torch.tensor([rp.lse], dtype=torch.float64)
        E_lse = GR.C_LSE * float(GR.t_lse(lse64, V))
        if math.isfinite(rp.lse):
            if abs(rp.lse) <= GR.NEAR:
                E_lse = min(E_lse, GR.LSE_GATE)
            assert abs(float(out["lse"][r]) - rp.lse) <= E_lse, (what, r, "lse", float(out["lse"][r]), rp.lse)
        else:
            assert float(out["lse"][r]) == rp.lse, (what, r, "lse")
        readings = [] if bad_params(t, k, p) else verify_row(rp, rq, d, t, k, p, key_accept, V)
        if not readings:
            assert tk == -1 and acc == 0 and out["logp"][r] == -np.inf and out["logq"][r] == -np.inf, (what, r, "empty row", tk, acc)
            continue
        draws += 1
        first = readings[0]
        undecided += not row_decided(readings, d)
        errs = []
        for rd in readings:
            e = _reading_error(rd, d, tk, acc, float(out["logq"][r]), float(out["log_ratio"][r]))
            if e is None:
                break
            errs.append(e)
        else:
            raise AssertionError((what, r, rp.stream, (t, k, p), d, tk, acc, errs[:2]))
        want_p = float(rp.xall[tk]) - rp.lse
        E_val = E_lse + U32 * (abs(want_p) + E_lse)
        if abs(rp.lse) <= GR.NEAR:
            E_val = min(E_val, GR.VAL_GATE)
        assert abs(float(out["logp"][r]) - want_p) <= E_val, (what, r, "logp", float(out["logp"][r]), want_p, E_val)
    return draws, undecided


def _reading_error(rd, d, tk, acc, logq, ratio):
    """None when the outputs satisfy the reading, else why not."""
    a = rd["a"]
    if math.isinf(a):
        if ratio != a:
            return ("log_ratio", ratio, a)
    elif not abs(ratio - a) <= rd["E_acc"]:
        return ("log_ratio", ratio, a, rd["E_acc"])
    if rd["acc_decided"] and acc != int(rd["accept"]):
        return ("accept", acc, rd["accept"], rd["logu"], a, rd["E_acc"])
    if acc:
        if tk != d:
            return ("accepted token", tk, d)
    elif tk not in rd["allowed"]:
        return ("residual token", tk, sorted(rd["allowed"])[:8], rd["res_token"])
    kp = rd["kp"]
    n = np.nonzero(kp["ids"] == tk)[0]
    if len(n) != 1:
        return ("token outside K_P", tk)
    if not abs(logq - float(kp["logr"][n[0]])) <= float(kp["E"][n[0]]):
        return ("logq", logq, float(kp["logr"][n[0]]), float(kp["E"][n[0]]))
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# one row, float32 in the kernel's order of operations
# ---------------------------------------------------------------------------------------------------------------------------
def verify_row_f32(rowp, rowq, d, temperature, top_k, top_p, key_accept, V):
    """-> dict(a, logu, accept, token, ids (K_P), v (perturbed residual values, -inf: no candidate), logq) or None (empty row)."""
    f32 = np.float32
    rp = SR.sample_row_f32(rowp, temperature, top_k, top_p)
    if rp["L"] == 0:
        return None
    L = rp["L"]
    ids = rowp.ids[:L]
    lp = rp["logq_all"].astype(f32)
    dd = ((rowp.x32[:L] - rowp.x32[0]).astype(f32) / f32(temperature)).astype(f32)
    lq = np.full(V, -np.inf, dtype=f32)
    if d != -1:
        rq = SR.sample_row_f32(rowq, temperature, top_k, top_p)
        if rq["L"]:
            lq[rowq.ids[:rq["L"]]] = rq["logq_all"].astype(f32)
    u = f32(accept_uniform(key_accept, rowp.stream))
    logu = f32(np.log(u))
    a = f32(-np.inf)
    pos = np.nonzero(ids == d)[0] if 0 <= d < V else []
    if len(pos):
        a = f32(lp[pos[0]] - lq[d]) if lq[d] > -np.inf else f32(np.inf)
    accept = bool(logu < a)
    inq = lq[ids] > -np.inf
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        rho = np.where(inq, np.exp((lq[ids] - lp).astype(f32)).astype(f32), f32(0.0))
        cand = rho < 1.0
        l1 = np.log1p(-np.where(cand, rho, f32(0.0))).astype(f32)
        v = ((dd + l1).astype(f32) + rowp.g32[:L]).astype(f32)
    v = np.where(cand, v, f32(-np.inf))
    if cand.any():
        best = np.nonzero(v == v.max())[0]
        tok = int(ids[best[np.argmin(ids[best])]])
    else:
        tok = int(ids[0])
    if accept:
        tok = d
    return dict(a=float(a), logu=float(logu), accept=accept, token=tok, ids=ids, v=v.astype(np.float64), rho=rho.astype(np.float64),
                logq=float(lp[np.nonzero(ids == tok)[0][0]]))


def measure_row(rowp, rowq, d, temperature, top_k, top_p, key_accept, V):
    """(accept, residual) ratios |float32 - float64| / (budget without its constant) of one row under its float64 reading; the
    residual ratio is taken over the ids that are candidates in both and whose float64 rho is certainly below one."""
    r32 = verify_row_f32(rowp, rowq, d, temperature, top_k, top_p, key_accept, V)
    rds = verify_row(rowp, rowq, d, temperature, top_k, top_p, key_accept, V) if r32 is not None else []
    if not rds or len(rds[0]["kp"]["ids"]) != len(r32["ids"]):
        return 0.0, 0.0
    rd, kp = rds[0], rds[0]["kp"]
    ra = 0.0
    if math.isfinite(rd["a"]) and math.isfinite(r32["a"]):
        ra = abs((r32["a"] - r32["logu"]) - (rd["a"] - rd["logu"])) / (rd["E_acc"] / C_ACC)
    kqs = kept_sets(rowq, temperature, top_k, top_p) if d != -1 else []
    lq, fq = _lookup(kqs[0] if kqs else None, V)
    ids, y, g = kp["ids"], kp["y"], kp["g"]
    lr = lq[ids] - kp["logr"]
    delta = SR.C_Q * U32 * (kp["form"] + fq[ids])
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        rho = np.exp(lr)
        ok = ((lr + delta < 0.0) | (lr == -np.inf)) & np.isfinite(r32["v"])
        rho = np.where(ok, rho, 0.0)
        l1 = np.log1p(-rho)
        w = (y - y[0]) + l1 + g
        E = U32 * ((1.0 + np.abs(y).max() + np.abs(g).max() + np.abs(l1)) + rho / (1.0 - rho) * (kp["form"] + fq[ids]))
    rr = float((np.abs(r32["v"] - w)[ok] / E[ok]).max()) if ok.any() else 0.0
    return ra, rr


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
PLANTED = ("xd equal to x", "d outside K_P", "d outside K_Q", "disjoint supports", "P <= Q on all ids but one", "ties in xd only",
           "-inf in xd only", "xd all -inf", "no draft", "d >= V", "d = -2")


@functools.lru_cache(maxsize=None)
def spec_case(V):
    """sample_ref.sample_case(V) (its planted rows: exact ties at the top-k boundaries and at the nucleus threshold, both flags,
    -inf logits, rows with nothing eligible, offsets) as the model's rows x; the draft's rows xd = x + noise (the ties and -inf
    of x survive where the noise is zero: every fourth row), and on the LAST len(PLANTED) rows (random ones of x) the planted
    relations of PLANTED -> dict(x, xd, flags, banned, streams, names, plant {name: row}, V)."""
    c = SR.sample_case(V, ROWS)
    g_ = torch.Generator().manual_seed(11 * V + 5)
    x = c["x"].clone()
    n = x.shape[0]
    noise = torch.randn(n, V, generator=g_) * 0.7
    noise[::4] = 0.0                                                     # these rows of xd equal x's: ties in both rows
    xd = x + noise
    names = list(c["names"])
    banned = set(int(b) for b in c["banned"].tolist())
    plant = {}
    ok = torch.tensor([i for i in range(V) if i != SEP and i not in banned])
    for off, name in enumerate(PLANTED):
        r = n - 1 - off
        assert names[r].startswith("random"), (V, r, names[r])
        assert int(c["flags"][r]) == 0
        plant[name] = r
        names[r] = name
        order = ok[torch.argsort(x[r][ok], descending=True, stable=True)]
        if name == "xd equal to x":
            xd[r] = x[r]
        elif name == "d outside K_Q":
            xd[r, order[0]] = -math.inf
        elif name == "disjoint supports":
            x[r, 0::2] = -math.inf                                       # K_P holds odd ids only, K_Q even ids only
            xd[r, 1::2] = -math.inf
        elif name == "P <= Q on all ids but one":
            xd[r] = x[r]
            xd[r, order[1]] -= 5.0
        elif name == "ties in xd only":
            xd[r] = c["x"][names.index("plateau on top")][torch.randperm(V, generator=g_)]
        elif name == "-inf in xd only":
            xd[r, torch.randperm(V, generator=g_)[:V // 4]] = -math.inf
        elif name == "xd all -inf":
            xd[r] = -math.inf
    return dict(x=x, xd=xd, flags=c["flags"], banned=c["banned"], streams=c["streams"], names=names, plant=plant, V=V)


@functools.lru_cache(maxsize=None)
def case_rows(V):
    """(Row of x keyed by KEY_RESIDUAL, Row of xd keyed by KEY_DRAFT) per row of spec_case(V)."""
    c = spec_case(V)
    mk = lambda a, key: [SR.Row(a[r], V, c["banned"], int(c["flags"][r]), SEP, key, int(c["streams"][r])) for r in range(a.shape[0])]   # noqa: E731
    rp, rq = mk(c["x"].numpy(), KEY_RESIDUAL), mk(c["xd"].numpy(), KEY_DRAFT)
    for r, (a, b) in enumerate(zip(rp, rq)):
        a.stream = b.stream = int(c["streams"][r])
    return rp, rq


def launch_params(V, launch_no, n=ROWS):
    """Per-row (temperature, top_k, top_p) of launch `launch_no`: row r takes combination 7 (r + launch_no n) mod 36 of
    TEMPS x TOP_KS x TOP_PS (7 and 36 are coprime: 36 consecutive rows see all of them)."""
    cs = [(t, k, p) for t in TEMPS for k in TOP_KS for p in TOP_PS]
    pick = [cs[(7 * (r + launch_no * n)) % len(cs)] for r in range(n)]
    return (np.array([c[0] for c in pick], dtype=np.float32), np.array([c[1] for c in pick], dtype=np.int32),
            np.array([c[2] for c in pick], dtype=np.float32))


LAUNCHES = 3


@functools.lru_cache(maxsize=None)
def drafts(V, launch_no):
    """The draft token of every row: the float64 mirror's draw from Q~ keyed by KEY_DRAFT (-1 where xd has nothing eligible),
    and the planted ones."""
    c = spec_case(V)
    rp, rq = case_rows(V)
    t, k, p = launch_params(V, launch_no)
    d = np.array([-1 if bad_params(t[r], k[r], p[r]) else SR.sample_row(rq[r], t[r], int(k[r]), p[r])["token"] for r in range(len(rq))],
                 dtype=np.int32)
    pl = c["plant"]
    d[pl["d outside K_P"]] = int(rp[pl["d outside K_P"]].ids[-1])       # the last id of P~'s rank order
    d[pl["d outside K_Q"]] = int(rp[pl["d outside K_Q"]].ids[0])        # P~'s first id, whose xd is -inf
    d[pl["xd all -inf"]] = int(rp[pl["xd all -inf"]].ids[0])
    d[pl["no draft"]] = -1
    d[pl["d >= V"]] = V + 3
    d[pl["d = -2"]] = -2
    d[3::16] = -1                                                        # and a few rows without a draft among the others
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# the rule against the two distributions (V small): the mirror of the kernel over many streams
# ---------------------------------------------------------------------------------------------------------------------------
def pair16():
    """The (x, xd) pair [16] of the distribution tests: overlapping supports, P~ > Q~ on some ids and < on others."""
    g_ = torch.Generator().manual_seed(1601)
    x = torch.randn(16, generator=g_) * 1.5
    xd = x + torch.randn(16, generator=g_)
    return x.numpy().astype(np.float32), xd.numpy().astype(np.float32)


def softmax_kept(x, t):
    y = np.asarray(x, dtype=np.float64) / t
    e = np.exp(y - y.max())
    return e / e.sum()


def mirror_streams(x, xd, t, streams, key_draft=KEY_DRAFT, key_accept=KEY_ACCEPT, key_residual=KEY_RESIDUAL):
    """The whole rule in float64 over `streams` (int array), no filtering, one (x, xd) pair [V]: the draft's Gumbel-max draw d,
    the accept test and the residual draw -> (accept [n] bool, token [n])."""
    V = len(x)
    ids = np.arange(V)
    P, Q = softmax_kept(x, t), softmax_kept(xd, t)
    lp, lq = np.log(P), np.log(Q)

    def noise(key):
        sk = np.array([SR.stream_key(key, int(s)) for s in streams], dtype=np.uint64)
        h = SR.mix32_np(sk[:, None] + ((ids.astype(np.uint64) * np.uint64(0x85EBCA77)) & SR.M32)[None])
        return ((h >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23

    d = np.argmax(lq[None] - np.log(-np.log(noise(key_draft))), 1)
    ua = noise(key_accept)[:, 0]
    acc = np.log(ua) < (lp - lq)[d]
    with np.errstate(divide="ignore"):
        res = np.where(P > Q, np.log(np.maximum(P - Q, 1e-300)), -np.inf)
    tok = np.argmax(res[None] - np.log(-np.log(noise(key_residual))), 1)
    return acc, np.where(acc, d, tok), d


def chi_square_cells(acc, tok, P, Q):
    """chi^2 of the 2 V cells (accept, token) against n min(P, Q) / n max(0, P - Q), cells with an expected count < 5 pooled
    -> (statistic, degrees of freedom)."""
    n, V = len(tok), len(P)
    obs = np.concatenate([np.bincount(tok[acc], minlength=V), np.bincount(tok[~acc], minlength=V)]).astype(np.float64)
    exp = np.concatenate([np.minimum(P, Q), np.maximum(0.0, P - Q)]) * n
    big = exp >= 5
    o, e = obs[big], exp[big]
    if (~big).any() and exp[~big].sum() > 0:
        o, e = np.append(o, obs[~big].sum()), np.append(e, exp[~big].sum())
    else:
        assert obs[~big].sum() == 0
    return float(((o - e) ** 2 / e).sum()), len(e) - 1
