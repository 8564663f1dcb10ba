"""unimm_lm_sample restated for the tests (TEST INFRASTRUCTURE): the host mirror of the kernel's uniforms, the float64 restatement
of one launch with its error budgets, and a float32 restatement in the kernel's order of operations that the budgets' constants
were measured with (the rule of oracle/generate_ref.py: a constant is the power of two >= 8 x the worst float32 / float64 ratio
over the suite's own cases, `sample_case`; tests/test_generate_sample_cpu.py prints the ratios again).

Semantics (include/unimm_hip.h), per row: eligible ids -> rank by (logit desc, id asc) -> the first min(top_k, n) -> y = x / t,
q ~ exp(y - max y) -> nucleus {x >= theta} -> token = argmax y + g (Gumbel-max) -> logq = y_t - logsumexp_kept y;
logp = x_t - logsumexp(x[:V]) and lse as in unimm_lm_topk (oracle.generate_ref.lm_topk's gates E_val / E_lse, unchanged).

Budgets (u = 2^-24):
  draw     A draw is DECIDED when the float64 gap between the best and the second-best perturbed value exceeds
           E_draw = C_DRAW u (1 + max |y| + max |g|) over the kept ids; a decided token must be the float64 argmax, an undecided
           one must be an id within E_draw of the best.  The kernel's value is fl(fl(fl(x - x_max) / t) - logf(-logf(u))): three
           roundings of magnitudes <= |y - y_max| and one of |g| / |y - y_max + g|, so the form covers it with room.
  nucleus  Id i stays iff A_i < top_p * total, A_i the mass of the kept logits strictly above x_i.  The kernel sums
           floor(expf(.) 2^40) in integers: each term is off by a few u relative (the rounded argument: u |y - y_max|, which
           weighted by q sums to at most u ln n, as for lse) plus 2^-40 absolute.  Membership is EXEMPT only when
           |A_i - top_p total| <= E_nuc = C_NUC u (1 + ln n) total, n the ids kept by top-k.
  logq     |err| <= E_logq = C_Q u (1 + ln n + |lse_y| + |logq|) with n the kept ids and lse_y = logsumexp_kept y: the form of
           E_val over the kept set (T_lse there, and u |val| for the value's own rounding).  Here |logq| is under the measured
           constant as well, because the token's y_t - y_max carries three roundings of that magnitude (the subtraction, the
           division by the temperature, the final subtraction), not the single one of x_t - lse.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from oracle import generate_ref as GR
from unimm_amd.dropout import mix32_int

U32 = 2.0 ** -24
FIX = 2.0 ** 40
SEP = GR.TOPK_SEP
M32 = np.uint64(0xFFFFFFFF)

# measured on the CPU over sample_case(V), V in SAMPLE_V, every (top_k, top_p, temperature) of the suite
# (tests/test_generate_sample_cpu.py::test_f32_restatement_inside_budgets prints them again):
DRAW_MEASURED = 2.641     # worst |fp32 perturbed value - fp64| / (u (1 + max |y| + max |g|))
C_DRAW = 32.0             # the power of two >= 8 x 2.641
NUC_MEASURED = 0.331      # worst |fp32 cumulative share - fp64| / (u (1 + ln n)) at the tie-group ends
C_NUC = 4.0               # the power of two >= 8 x 0.331
Q_MEASURED = 1.758        # worst |fp32 logq - fp64| / (u (1 + ln n + |lse_y| + |logq|)) over every kept id
C_Q = 16.0                # the power of two >= 8 x 1.758

CASE_KEY = 0x5A17C0DE
SAMPLE_V = GR.TOPK_V                              # (16, 255, 256, 257, 1000, 30522, 65536)
TEMPS = (1.0, 0.7, 2.0)
TOP_PS = (1.0, 0.9, 0.5, 1e-6)
ROWS = 64


def top_ks(V):
    return (0, 1, 2, 50, V)


# ---------------------------------------------------------------------------------------------------------------------------
# the uniforms
# ---------------------------------------------------------------------------------------------------------------------------
def mix32_np(x):
    """unimm_amd.dropout.mix32_int on a uint64 array of 32-bit words."""
    x = x & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def stream_key(key, stream):
    return mix32_int((key & 0xFFFFFFFF) ^ (((stream & 0xFFFFFFFF) * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF))


def hashes(key, stream, ids):
    """h_i of the header for the ids (any integer array) -> uint64 array of 32-bit words."""
    sk = np.uint64(stream_key(int(key), int(stream)))
    i = np.asarray(ids).astype(np.uint64)
    return mix32_np(sk + ((i * np.uint64(0x85EBCA77)) & M32))


def uniforms(key, stream, ids):
    """u_i = ((h_i >> 9) + 0.5) 2^-23, float64 (exact; the same number in float32)."""
    return ((hashes(key, stream, ids) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel64(key, stream, ids):
    return -np.log(-np.log(uniforms(key, stream, ids)))


def gumbel32(key, stream, ids):
    u = uniforms(key, stream, ids).astype(np.float32)
    return (-np.log((-np.log(u)).astype(np.float32))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# one row, float64
# ---------------------------------------------------------------------------------------------------------------------------
class Row:
    """What does not depend on (top_k, top_p, temperature): the eligible ids in rank order, their logits, tie groups and noise."""

    def __init__(self, x, V, banned, flag, sep, key, stream):
        x = np.asarray(x[:V], dtype=np.float32)
        with np.errstate(invalid="ignore"):
            elig = ~GR.banned_mask(V, banned, int(flag), sep) & (x > -np.inf)
        ids = np.nonzero(elig)[0]
        xe = x[ids] + np.float32(0.0)                              # -0 -> +0
        o = np.lexsort((ids, -xe))
        self.ids = ids[o].astype(np.int64)
        self.x32 = xe[o]
        self.x = self.x32.astype(np.float64)
        n = self.n = len(self.ids)
        new = np.ones(n, dtype=bool)
        new[1:] = self.x32[1:] != self.x32[:-1]
        self.gstart = np.maximum.accumulate(np.where(new, np.arange(n), 0))           # first rank of the tie group
        nxt = np.append(np.nonzero(new)[0][1:], n) if n else np.zeros(0, dtype=np.int64)
        self.gend = nxt[np.cumsum(new) - 1] if n else nxt                              # one past its last rank
        self.g = gumbel64(key, stream, self.ids)
        self.g32 = gumbel32(key, stream, self.ids)
        with np.errstate(over="ignore"):
            self.lse = float(torch.logsumexp(torch.from_numpy(x.astype(np.float64)), 0))
        self.xall = x


def sample_row(row, temperature, top_k, top_p):
    """float64 restatement of one row -> dict: token, logp, logq (of the float64 kept set), decided, gap, E_draw, lengths (the
    admissible sizes of the kept set: one unless a nucleus membership is exempt), allowed = {id: [(logq, E_logq) per admissible
    kept set that has the id within E_draw of its best]}."""
    t, p = float(np.float32(temperature)), float(np.float32(top_p))
    n = row.n
    if n == 0:
        return dict(token=-1, logp=-math.inf, logq=-math.inf, allowed={}, decided=True, lengths=[], n=0)
    nk = min(int(top_k), n) if top_k > 0 else n
    y = row.x[:nk] / t
    q = np.exp(y - y[0])
    cum = np.cumsum(q)
    total = cum[-1]
    lengths = [nk]
    if p < 1.0:
        A = np.where(row.gstart[:nk] > 0, cum[np.maximum(row.gstart[:nk], 1) - 1], 0.0)
        member = A < p * total
        member[0] = True
        L = int(member.sum())
        lengths = [L]
        E_nuc = C_NUC * U32 * (1.0 + math.log(nk)) * total
        for b in np.nonzero((np.abs(A - p * total) <= E_nuc) & (row.gstart[:nk] == np.arange(nk)) & (np.arange(nk) > 0))[0]:
            for cand in (int(b), min(int(row.gend[b]), nk)):
                if cand not in lengths:
                    lengths.append(cand)
    Lmin, Lmax = min(lengths), max(lengths)
    # the draw is judged on the largest admissible kept set: decided when its best id is a certain member (rank < Lmin) and leads
    # by more than E_draw; the admissible tokens are the ids within E_draw of the best of ANY admissible kept set
    vmax = y[:Lmax] + row.g[:Lmax]
    best = float(vmax.max())
    top = np.nonzero(vmax == best)[0]
    it = int(top[np.argmin(row.ids[top])])
    second = float(np.partition(vmax, Lmax - 2)[Lmax - 2]) if Lmax > 1 else -math.inf
    E_draw = C_DRAW * U32 * (1.0 + float(np.abs(y[:Lmax]).max()) + float(np.abs(row.g[:Lmax]).max()))
    decided = len(top) == 1 and it < Lmin and best - second > E_draw
    allowed = {}
    for L in lengths:
        v = vmax[:L]
        lse_y = y[0] + math.log(float(cum[L - 1]))
        for i in np.nonzero(v >= float(v.max()) - E_draw)[0]:
            lq = float(y[i] - lse_y)
            allowed.setdefault(int(row.ids[i]), []).append((lq, C_Q * U32 * (1.0 + math.log(L) + abs(lse_y) + abs(lq))))
    L0 = lengths[0]
    v0 = vmax[:L0]
    t0 = np.nonzero(v0 == v0.max())[0]
    tok = int(row.ids[int(t0[np.argmin(row.ids[t0])])])
    return dict(token=tok, logp=float(row.xall[tok]) - row.lse, logq=allowed[tok][0][0], allowed=allowed, decided=decided,
                gap=best - second, E_draw=E_draw, lengths=lengths, n=nk)


# ---------------------------------------------------------------------------------------------------------------------------
# one row, float32 in the kernel's order of operations
# ---------------------------------------------------------------------------------------------------------------------------
def sample_row_f32(row, temperature, top_k, top_p):
    """-> dict(token, logq (of that token), L, v float32 [L] relative to y_max, fixcum int [nk], ztot): the kernel's arithmetic --
    d = fl(fl(x - x_max) / t), masses floor(expf(d) 2^40) summed as integers, target ceil(double(top_p) * double(total)),
    v = fl(d - logf(-logf(u))), logq = fl(d_t - logf(fl32(double(zf) 2^-40)))."""
    f32 = np.float32
    t, p = f32(temperature), f32(top_p)
    n = row.n
    if n == 0:
        return dict(token=-1, logq=-math.inf, L=0)
    nk = min(int(top_k), n) if top_k > 0 else n
    d = ((row.x32[:nk] - row.x32[0]).astype(f32) / t).astype(f32)
    with np.errstate(under="ignore"):
        e = np.exp(d).astype(f32)
    fix = np.floor(e.astype(np.float64) * FIX).astype(np.uint64)
    cum = np.cumsum(fix)
    L = nk
    if float(p) < 1.0 and n > 1:
        target = max(1, math.ceil(float(p) * float(int(cum[-1]))))
        ends = row.gend[:nk].clip(max=nk)
        reach = cum[ends - 1] >= np.uint64(target)
        L = int(ends[int(np.argmax(reach))]) if reach.any() else nk
    v = (d[:L] + row.g32[:L]).astype(f32)
    best = v.max()
    top = np.nonzero(v == best)[0]
    it = int(top[np.argmin(row.ids[top])])
    zf = f32(float(int(cum[L - 1])) * 2.0 ** -40)
    logq = (d[:L] - np.log(zf).astype(f32)).astype(f32)
    return dict(token=int(row.ids[it]), logq=float(logq[it]), logq_all=logq.astype(np.float64), L=L, v=v.astype(np.float64),
                fixcum=cum, nk=nk)


def measure_row(row, temperature, top_k, top_p, r32=None):
    """(draw, nucleus, logq) ratios |float32 - float64| / (budget form without its constant) of one row."""
    n = row.n
    if n == 0:
        return 0.0, 0.0, 0.0
    t = float(np.float32(temperature))
    r32 = sample_row_f32(row, temperature, top_k, top_p) if r32 is None else r32
    nk, L = r32["nk"], r32["L"]
    y = row.x[:nk] / t
    q = np.exp(y - y[0])
    cum = np.cumsum(q)
    # nucleus: the cumulative share at every tie-group end
    ends = np.unique(row.gend[:nk].clip(max=nk))
    share32 = r32["fixcum"][ends - 1].astype(np.float64) / float(int(r32["fixcum"][-1]))
    rn = float(np.abs(share32 - cum[ends - 1] / cum[-1]).max() / (U32 * (1.0 + math.log(nk))))
    # draw: perturbed values relative to y_max, over the float32 kept set
    v64 = (y[:L] - y[0]) + row.g[:L]
    rd = float(np.abs(r32["v"] - v64).max() / (U32 * (1.0 + float(np.abs(y[:L]).max()) + float(np.abs(row.g[:L]).max()))))
    lse_y = y[0] + math.log(float(cum[L - 1]))
    lq = y[:L] - lse_y
    rq = float((np.abs(r32["logq_all"] - lq) / (U32 * (1.0 + math.log(L) + abs(lse_y) + np.abs(lq)))).max())
    return rd, rn, rq


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sample_case(V, rows=ROWS):
    """The planted rows of oracle.generate_ref.topk_case(V) (random, exact ties, both flags, -inf logits, +-1e4 offsets, banned ids
    on top) with a banned list of its own (duplicates, ids outside [0, V)), plateaus across the top-k boundaries and at the nucleus
    threshold, a row of -inf only, and random rows up to `rows` -> dict(x fp32 [rows, V], flags, banned, streams, names)."""
    tc = GR.topk_case(V)
    g_ = torch.Generator().manual_seed(7 * V + 1)
    rnd = lambda s=3.0: torch.randn(V, generator=g_) * s         # noqa: E731
    xs, flags, names = list(tc["x"]), tc["flags"].tolist(), list(tc["names"])

    def add(name, x, f=0):
        names.append(name); xs.append(x.float()); flags.append(f)

    # the launch's banned list: the default ids, the top four of the "banned ids on top" row, duplicates, negatives, ids >= V
    top = torch.topk(tc["x"][tc["names"].index("banned ids on top")], min(4, V)).indices.to(torch.int32)
    banned = torch.cat([torch.tensor([0, 101 % V, 103 % V], dtype=torch.int32), top, tc["banned"][80:100], top[:2],
                        torch.tensor([0, V, -1], dtype=torch.int32)])
    perm = torch.tensor([i for i in torch.randperm(V, generator=g_).tolist() if i != SEP and i not in banned.tolist()])   # planted ids: eligible ones
    x = rnd()
    x[perm[:min(70, V // 2)]] = 30.0                             # top_k = 2 and 50 cut inside the plateau: the id decides
    add("plateau on top", x)
    x = rnd()
    x[perm[0]] = 31.0
    x[perm[1:4]] = 30.0                                          # ranks 1 .. 3 tie: top_k = 2 takes the smallest id of them
    add("plateau at ranks 1-3", x)
    x = rnd() - 40.0
    x[perm[0]] = 1.0
    x[perm[1:9]] = 0.0                                           # top holds < half of the mass at every temperature: theta = 0,
    add("plateau at the nucleus threshold", x)                   # and all eight tied ids stay
    x = rnd()
    x[perm[2]] = -0.0
    x[perm[3]] = 0.0
    add("signed zeros", x)
    add("all -inf", torch.full((V,), -math.inf))
    add("all -inf, sep forced", torch.full((V,), -math.inf), 2)
    x = rnd(1.0)
    add("flat", x)
    while len(xs) < rows:
        add("random %d" % len(xs), rnd(1.5 if len(xs) % 2 else 3.0))
    streams = torch.arange(len(xs), dtype=torch.int32) * 7919 + V
    streams[1] = -5                                              # a negative stream id is a 32-bit word like any other
    # The rows offset by +-1e4 have max |y| ~ 1e4, hence E_draw ~ 2e-2: about one stream in fifty leaves such a draw undecided
    # by definition, whatever the kernel does.  The cap on undecided draws is a condition on the inputs: take, for these
    # rows, the first stream of a fixed sequence whose draws the float64 restatement decides for every setting of the suite.
    for r, name in enumerate(names):
        if name.startswith("offset"):
            for j in range(64):
                st = int(streams[r]) + 104729 * j
                row = Row(xs[r].numpy(), V, banned, flags[r], SEP, CASE_KEY, st)
                if all(sample_row(row, t, k, p)["decided"] for k, p, t in combos(V)):
                    break
            streams[r] = st
    return dict(x=torch.stack(xs), flags=torch.tensor(flags, dtype=torch.int32), banned=banned, streams=streams, names=names, V=V)


def case_rows(case, key=CASE_KEY):
    x = case["x"].numpy()
    return [Row(x[r], case["V"], case["banned"], int(case["flags"][r]), SEP, key, int(case["streams"][r])) for r in range(x.shape[0])]


def combos(V):
    return [(k, p, t) for k in top_ks(V) for p in TOP_PS for t in TEMPS]


def measure(vs=SAMPLE_V, combos_of=combos):
    """Worst (draw, nucleus, logq) ratios over the suite's cases."""
    w = np.zeros(3)
    for V in vs:
        rows = case_rows(sample_case(V))
        for k, p, t in combos_of(V):
            for row in rows:
                w = np.maximum(w, measure_row(row, t, k, p))
    return tuple(float(a) for a in w)


def pow2_at_least(v):
    return 2.0 ** math.ceil(math.log2(v))


# ---------------------------------------------------------------------------------------------------------------------------
# checking one launch
# ---------------------------------------------------------------------------------------------------------------------------
def check_rows(rows, V, temperature, top_k, top_p, token, logp, logq, lse, what=""):
    """token / logp / logq / lse: the kernel's outputs (host arrays) for the Row objects -> (draws, undecided, worst ratios)."""
    draws = undecided = 0
    worst = np.zeros(3)
    for r, row in enumerate(rows):
        ref = sample_row(row, temperature, top_k, top_p)
        tk = int(token[r])
        lse64 = torch.tensor([row.lse], dtype=torch.float64)
        E_lse = GR.C_LSE * float(GR.t_lse(lse64, V))
        if math.isfinite(row.lse):
            if abs(row.lse) <= GR.NEAR:
                E_lse = min(E_lse, GR.LSE_GATE)
            el = abs(float(lse[r]) - row.lse)
            assert el <= E_lse, (what, r, "lse", float(lse[r]), row.lse, E_lse)
            worst[0] = max(worst[0], el / E_lse)
        else:
            assert float(lse[r]) == row.lse, (what, r, "lse", float(lse[r]), row.lse)
        if ref["token"] < 0:
            assert tk == -1 and float(logp[r]) == -math.inf and float(logq[r]) == -math.inf, (what, r, tk)
            continue
        draws += 1
        if ref["decided"]:
            assert tk == ref["token"], (what, r, "decided draw", tk, ref["token"], ref["gap"], ref["E_draw"])
        else:
            undecided += 1
            assert tk in ref["allowed"], (what, r, "token outside the ids within E_draw of the best", tk, ref["token"])
        rq = min(abs(float(logq[r]) - lq) / E for lq, E in ref["allowed"][tk])
        assert rq <= 1.0, (what, r, "logq", float(logq[r]), ref["allowed"][tk], rq)
        worst[2] = max(worst[2], rq)
        want_p = float(row.xall[tk]) - row.lse
        E_val = E_lse + U32 * (abs(want_p) + E_lse)
        if abs(row.lse) <= GR.NEAR:
            E_val = min(E_val, GR.VAL_GATE)
        ep = abs(float(logp[r]) - want_p)
        assert ep <= E_val, (what, r, "logp", float(logp[r]), want_p, E_val)
        worst[1] = max(worst[1], ep / E_val)
    return draws, undecided, worst


# ---------------------------------------------------------------------------------------------------------------------------
# the mirrored generator against the softmax
# ---------------------------------------------------------------------------------------------------------------------------
def chi_square(V, streams, scale=1.5, key=CASE_KEY, seed=0):
    """Draws of the mirror (float64 Gumbel-max, no filtering) from one row randn * scale over `streams` streams -> (chi^2 against
    the softmax over the ids with an expected count >= 5 (the others pooled), its degrees of freedom, draws with a top-2 gap below
    1e-4, smallest gap)."""
    x = (torch.randn(V, generator=torch.Generator().manual_seed(seed)) * scale).numpy().astype(np.float64)
    mul = (np.arange(V, dtype=np.uint64) * np.uint64(0x85EBCA77)) & M32
    sk = np.array([stream_key(key, s) for s in range(streams)], dtype=np.uint64)
    counts = np.zeros(V)
    small, gmin = 0, math.inf
    for c0 in range(0, streams, 4096):
        h = mix32_np(sk[c0:c0 + 4096, None] + mul[None, :])
        u = ((h >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        v = x[None, :] - np.log(-np.log(u))
        top2 = np.partition(v, V - 2, axis=1)[:, V - 2:]
        gap = top2[:, 1] - top2[:, 0]
        small += int((gap < 1e-4).sum())
        gmin = min(gmin, float(gap.min()))
        counts += np.bincount(np.argmax(v, axis=1), minlength=V)
    pr = np.exp(x - x.max())
    pr /= pr.sum()
    exp = pr * streams
    big = exp >= 5
    obs, ex = counts[big], exp[big]
    if (~big).any():
        obs, ex = np.append(obs, counts[~big].sum()), np.append(ex, exp[~big].sum())
    return float(((obs - ex) ** 2 / ex).sum()), len(ex) - 1, small, gmin


def chi_square_critical(df, z=3.0902):
    """The 0.1 % critical value of chi^2 with df degrees of freedom (Wilson-Hilferty; within 0.5 % of the tables for df >= 10)."""
    return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3
