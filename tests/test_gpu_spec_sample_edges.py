"""unimm_lm_spec_verify (the rejection step of speculative sampling) at its edges, through the C ABI, per element against
tests/spec_sample_ref.py: V in (16, 257, 30522, 65536) -- both the LDS-staged and the re-read path -- 64 rows, per-row
temperature in (1, 0.7, 2) x top_k in (0, 1, 2, 50) x top_p in (1, 0.9, 1e-6) mixed within each launch, the planted rows of
spec_sample_ref.spec_case (xd equal to x, d outside K_P / K_Q, disjoint supports, P~ <= Q~ on all ids but one, exact ties at the
top-k boundary and the nucleus threshold in either row, -inf logits in either row, both flags, nothing eligible, d = -1, d >= V),
NaN past V and around the rows.

(a) every launch against the float64 restatement, with the cap on undecided rows the CPU suite meets by the reference alone;
(i) rows with d = -1 equal unimm_lm_sample_rows keyed by key_residual bit for bit; (ii) xd the same buffer as x: log_ratio == 0
and accept = 1 wherever d is in K_P; (iii) top_k = 1 rows are unimm_lm_topk's first id with logq = 0 and accept = (d == id),
whatever the keys; (iv) a row does not depend on its position, the number of rows or the other rows; bad per-row parameters;
the refusals and rows = 0; and the rule against min(P~, Q~) / max(0, P~ - Q~) over 65,536 streams on the device."""
import numpy as np
import pytest
import torch

from oracle import generate_ref as GR
from tests import sample_ref as SR
from tests import spec_sample_ref as R

pytestmark = pytest.mark.gpu
GUARD = GR.GUARD
SENT = -768.0
DEV = "cuda"
NAMES = ("accept", "token", "logp", "logq", "lse", "log_ratio")


def padded(a, V, ld):
    n = a.shape[0]
    b = torch.full((GUARD + n + GUARD, ld), float("nan"), dtype=torch.float32)
    b[GUARD:GUARD + n, :V] = a
    return b.to(DEV)[GUARD:GUARD + n]


class Buffers:
    """spec_case(V) on the device: both logits tables inside NaN guard rows with NaN columns past V, sentinel-filled outputs."""

    def __init__(self, V):
        c = self.case = R.spec_case(V)
        self.V, self.n = V, c["x"].shape[0]
        self.x = padded(c["x"], V, (V + 63) // 64 * 64 + 64)
        self.xd = padded(c["xd"], V, V + 3)
        self.banned, self.flags, self.streams = (c[k].to(DEV) for k in ("banned", "flags", "streams"))
        self.rows = R.case_rows(V)

    def launch(self, params, draft, x=None, xd=None, keys=(R.KEY_ACCEPT, R.KEY_RESIDUAL), rows=None, sel=None, ratio=True):
        """One unimm_lm_spec_verify launch on the rows `sel` (default: all, in order) -> dict of host arrays."""
        from unimm_amd import lib as SP
        x, xd = self.x if x is None else x, self.xd if xd is None else xd
        flags, streams = self.flags, self.streams
        t, k, p, d = (torch.as_tensor(a) for a in (*params, draft))
        if sel is not None:
            idx = torch.as_tensor(sel)
            x, xd = x[idx.to(DEV)].contiguous(), xd[idx.to(DEV)].contiguous()
            flags, streams = flags[idx.to(DEV)], streams[idx.to(DEV)]
            t, k, p, d = t[idx], k[idx], p[idx], d[idx]
        n = x.shape[0]
        rows = n if rows is None else rows
        N = GUARD + n + GUARD
        ints = [torch.full((N,), -7, dtype=torch.int32, device=DEV) for _ in range(2)]
        flts = [torch.full((N,), SENT, dtype=torch.float32, device=DEV) for _ in range(4)]
        b = slice(GUARD, GUARD + n)
        SP.lm_spec_verify(x, xd, rows, self.V, d.to(DEV, torch.int32), self.banned, flags, SR.SEP, t.to(DEV, torch.float32),
                          k.to(DEV, torch.int32), p.to(DEV, torch.float32), keys[0], keys[1], streams, ints[0][b], ints[1][b],
                          flts[0][b], flts[1][b], flts[2][b], flts[3][b] if ratio else None)
        torch.cuda.synchronize()
        out = {}
        for name, o in zip(NAMES, ints + flts):
            o = o.cpu()
            keep = torch.ones(N, dtype=torch.bool)
            keep[GUARD:GUARD + rows] = False
            assert (o[keep] == (-7 if o.dtype == torch.int32 else SENT)).all(), (name, "wrote outside its rows")
            out[name] = o[GUARD:GUARD + rows].numpy()
        assert not np.isnan(out["logp"]).any() and not np.isnan(out["logq"]).any() and not np.isnan(out["log_ratio"] if ratio else 0).any()
        return out

    def sample_rows(self, params, key, x=None):
        """unimm_lm_sample_rows on the model's rows -> (token, logp, logq, lse) host arrays."""
        from unimm_amd import lib as L
        n = self.n
        tok = torch.empty(n, dtype=torch.int32, device=DEV)
        lp, lq, lse = (torch.empty(n, dtype=torch.float32, device=DEV) for _ in range(3))
        t, k, p = (torch.as_tensor(a).to(DEV) for a in params)
        L.lm_sample_rows(self.x if x is None else x, n, self.V, self.banned, self.flags, SR.SEP, t, k, p, key, self.streams, tok, lp, lq, lse)
        torch.cuda.synchronize()
        return tuple(a.cpu().numpy() for a in (tok, lp, lq, lse))


def bits(a):
    return a.view(np.int32)


def same(a, b, rows=slice(None), names=NAMES, what=""):
    for name in names:
        assert np.array_equal(bits(a[name])[rows], bits(b[name])[rows]), (what, name, np.nonzero(bits(a[name])[rows] != bits(b[name])[rows])[0][:8])


@pytest.mark.parametrize("V", R.SPEC_V)
def test_every_row_against_the_float64_restatement(V):
    b = Buffers(V)
    rp, rq = b.rows
    names = b.case["names"]
    plain = np.array([nm.startswith("random") for nm in names])
    draws = undecided = 0
    for no in range(R.LAUNCHES):
        params, d = R.launch_params(V, no), R.drafts(V, no)
        out = b.launch(params, d)
        n, u = R.check_launch(rp, rq, d, params, R.KEY_ACCEPT, V, out, what=f"V {V} launch {no}")
        sel = np.nonzero(plain)[0]
        n2, u2 = R.check_launch([rp[r] for r in sel], [rq[r] for r in sel], d[sel], tuple(a[sel] for a in params), R.KEY_ACCEPT, V,
                                {k: v[sel] for k, v in out.items()})
        draws, undecided = draws + n2, undecided + u2
        assert ((out["token"] >= -1) & (out["token"] < V)).all()
        pl = b.case["plant"]
        r = pl["d outside K_P"]
        if params[1][r] in (1, 2) and rp[r].n > 2:
            assert out["accept"][r] == 0 and out["log_ratio"][r] == -np.inf
        assert out["accept"][pl["d outside K_Q"]] == 1 and out["log_ratio"][pl["d outside K_Q"]] == np.inf
        assert out["accept"][pl["xd all -inf"]] == 1
        for nm in ("no draft", "d >= V", "d = -2"):
            assert out["accept"][pl[nm]] == 0 and out["log_ratio"][pl[nm]] == -np.inf and out["token"][pl[nm]] >= 0
        r = pl["disjoint supports"]
        assert out["token"][r] % 2 == 1 and (out["accept"][r] == 0 or d[r] == -1)
    print(f"\nlm_spec_verify V = {V}: {undecided} of {draws} non-planted rows undecided in the float64 restatement")
    assert draws > 60 and undecided <= R.UNDECIDED_CAP * draws


@pytest.mark.parametrize("V", R.SPEC_V)
def test_rows_without_a_draft_are_the_samplers(V):
    """(i), with every row's draft taken away; lse and logp of ALL rows of a drafted launch are the sampler's too."""
    b = Buffers(V)
    params = R.launch_params(V, 1)
    none = np.full(b.n, -1, dtype=np.int32)
    out = b.launch(params, none, keys=(123, R.KEY_RESIDUAL))
    tok, lp, lq, lse = b.sample_rows(params, R.KEY_RESIDUAL)
    diff = {name: np.nonzero(bits(out[name]) != bits(want))[0][:8].tolist()
            for name, want in zip(("token", "logp", "logq", "lse"), (tok, lp, lq, lse)) if not np.array_equal(bits(out[name]), bits(want))}
    assert not diff, (diff, {name: (out[name][r[0]], want[r[0]]) for (name, r), want in zip(diff.items(), (tok, lp, lq, lse))})
    assert (out["accept"] == 0).all() and (out["log_ratio"] == -np.inf).all()
    d = R.drafts(V, 1)
    mixed = b.launch(params, d)
    nod = d == -1
    assert nod.sum() >= 4
    same(mixed, out, rows=nod, names=("token", "logp", "logq", "lse", "accept", "log_ratio"))
    assert np.array_equal(bits(mixed["lse"]), bits(lse))
    noratio = b.launch(params, d, ratio=False)
    same(noratio, mixed, names=NAMES[:5])


@pytest.mark.parametrize("V", R.SPEC_V)
def test_same_buffer_accepts_with_ratio_zero(V):
    """(ii): xd is x's buffer; d = the sampler's own draw from x (inside K_P by construction), keyed by the draft's key."""
    b = Buffers(V)
    for no in range(2):
        params = R.launch_params(V, no)
        d = b.sample_rows(params, R.KEY_DRAFT)[0]
        out = b.launch(params, d, xd=b.x)
        live = d >= 0
        assert live.sum() >= b.n - 12
        assert (out["log_ratio"][live] == 0.0).all() and (out["accept"][live] == 1).all() and (out["token"][live] == d[live]).all()
        plain = b.sample_rows(params, R.KEY_DRAFT)
        assert np.array_equal(bits(out["logp"]), bits(plain[1])) and np.array_equal(bits(out["logq"]), bits(plain[2]))


@pytest.mark.parametrize("V", R.SPEC_V)
def test_greedy_rows_are_lm_topk(V):
    """(iii)"""
    from unimm_amd import lib as L
    b = Buffers(V)
    n = b.n
    vals = torch.empty((n, 1), dtype=torch.float32, device=DEV)
    ids = torch.empty((n, 1), dtype=torch.int32, device=DEV)
    L.lm_topk(b.x, n, V, b.banned, b.flags, SR.SEP, 1, vals, ids)
    idd = torch.empty((n, 1), dtype=torch.int32, device=DEV)
    L.lm_topk(b.xd, n, V, b.banned, b.flags, SR.SEP, 1, torch.empty_like(vals), idd)
    torch.cuda.synchronize()
    vals, ids, idd = vals.cpu().numpy()[:, 0], ids.cpu().numpy()[:, 0], idd.cpu().numpy()[:, 0]
    t, k, p = R.launch_params(V, 2)
    k = np.ones_like(k)
    d = np.where(np.arange(n) % 3 == 0, ids, idd).astype(np.int32)      # the model's id, or the draft's (often another)
    d[5::7] = -1
    a = b.launch((t, k, p), d)
    c = b.launch((t, k, p), d, keys=(77, 99))
    same(a, c, what="the keys matter on a greedy row")
    some = vals > -np.inf
    assert some.sum() >= n - 8 and (a["token"][~some] == -1).all() and (a["accept"][~some] == 0).all()
    assert np.array_equal(a["token"][some], ids[some]) and (a["logq"][some] == 0.0).all()
    assert np.array_equal(bits(a["logp"][some]), bits(vals[some]))
    assert np.array_equal(a["accept"][some], (d == ids)[some].astype(np.int32)) and (d == ids)[some].sum() >= n // 3 - 8
    assert (d != ids)[some].sum() >= 4


@pytest.mark.parametrize("V", R.SPEC_V)
def test_a_row_depends_on_its_own_inputs_alone(V):
    """(iv): a launch repeats; rows in another order, fewer rows, one row alone, and other rows' parameters changed."""
    b = Buffers(V)
    n = b.n
    params, d = R.launch_params(V, 0), R.drafts(V, 0)
    a = b.launch(params, d)
    same(b.launch(params, d), a, what="repeated launch")
    perm = np.roll(np.arange(n), 17)[::-1].copy()
    moved = b.launch(params, d, sel=perm)
    for name in NAMES:
        assert np.array_equal(bits(moved[name]), bits(a[name])[perm]), ("permuted rows", name)
    part = b.launch(params, d, rows=5)
    same(part, {k: v[:5] for k, v in a.items()}, what="fewer rows")
    r = b.case["plant"]["P <= Q on all ids but one"]
    one = b.launch(params, d, sel=[r])
    same(one, {k: v[r:r + 1] for k, v in a.items()}, what="one row alone")
    t, k, p = (x.copy() for x in params)
    fixed = np.arange(n) % 4 == 0
    t[~fixed], k[~fixed], p[~fixed] = 1.5, 3, 0.8
    d2 = d.copy()
    d2[~fixed] = 1
    same(b.launch((t, k, p), d2), a, rows=fixed, what="other rows' parameters and drafts")
    other = b.launch(params, d, keys=(R.KEY_ACCEPT + 1, R.KEY_RESIDUAL + 1))
    assert (other["token"] != a["token"]).any()


INVALID = [(0.0, 0, 1.0), (-1.0, 0, 1.0), (float("nan"), 0, 1.0), (float("inf"), 0, 1.0), (1.0, 0, 0.0), (1.0, 0, 1.5),
           (1.0, 0, float("nan")), (1.0, -1, 1.0), (0.7, -2 ** 31, 0.9)]


@pytest.mark.parametrize("V", (257, 65536))
def test_invalid_rows_and_rows_with_nothing_eligible(V):
    b = Buffers(V)
    n = b.n
    params, d = R.launch_params(V, 0), R.drafts(V, 0)
    good = b.launch(params, d)
    t, k, p = (a.copy() for a in params)
    bad = np.zeros(n, dtype=bool)
    for i, (ti, ki, pi) in enumerate(INVALID):
        r = (4 * i + 1) % n
        t[r], k[r], p[r] = ti, ki, pi
        bad[r] = True
    got = b.launch((t, k, p), d)
    assert (got["token"][bad] == -1).all() and (got["accept"][bad] == 0).all()
    assert (got["logp"][bad] == -np.inf).all() and (got["logq"][bad] == -np.inf).all()
    assert np.array_equal(bits(got["lse"]), bits(good["lse"]))
    same(got, good, rows=~bad, what="rows next to invalid ones")
    empty = np.array([r.n == 0 for r in b.rows[0]])
    assert empty.sum() >= 3
    assert (good["token"][empty] == -1).all() and (good["accept"][empty] == 0).all() and (good["logq"][empty] == -np.inf).all()
    flags = b.case["flags"].numpy()
    live = ((flags & 2) != 0) & ~empty
    if V > SR.SEP:
        assert live.sum() >= 1 and (good["token"][live] == SR.SEP).all() and (good["logq"][live] == 0.0).all()
        assert np.array_equal(good["accept"][live], (d[live] == SR.SEP).astype(np.int32))
        sep_d = d.copy()
        sep_d[live] = SR.SEP
        assert (b.launch(params, sep_d)["accept"][live] == 1).all()
    assert (good["token"][(flags & 1) != 0] != SR.SEP).all()


def test_refusals_and_zero_rows():
    from unimm_amd import lib as L
    from unimm_amd import lib as SP
    V = 257
    b = Buffers(V)
    n = b.n
    t, k, p = (torch.as_tensor(a).to(DEV) for a in R.launch_params(V, 0))
    d = torch.as_tensor(R.drafts(V, 0)).to(DEV)
    acc, tok = (torch.full((n,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    lp, lq, lse, ratio = (torch.full((n,), SENT, dtype=torch.float32, device=DEV) for _ in range(4))
    args = [b.x, b.xd, n, V, d, None, None, SR.SEP, t, k, p, 1, 2, b.streams, acc, tok, lp, lq, lse, ratio]
    for i in (0, 1, 4, 8, 9, 10, 13, 14, 15, 16, 17, 18):
        broken = list(args)
        broken[i] = None
        with pytest.raises(L.UnimmHipError, match="UNIMM_E_ARG"):
            SP.lm_spec_verify(*broken)
    for i, v in ((3, 0), (3, 65537), (3, V + 200), (2, -1)):
        broken = list(args)
        broken[i] = v
        with pytest.raises(L.UnimmHipError, match="UNIMM_E_SHAPE"):
            SP.lm_spec_verify(*broken)
    args[2] = 0
    SP.lm_spec_verify(*args)
    torch.cuda.synchronize()
    assert (acc == -7).all() and (tok == -7).all() and all((a == SENT).all() for a in (lp, lq, lse, ratio))


def test_the_rule_against_both_distributions_on_the_device():
    """V = 16, 65,536 rows that share one (x, xd) pair, streams 0 .. 65535, d drawn per row by the draft-side launch
    (unimm_lm_sample_rows on xd): chi^2 over the cells (accept, token) against n min(P~, Q~) / n max(0, P~ - Q~), cells with an
    expected count below 5 pooled, below the 0.1 % critical value.  The mirror passes with the same keys on the CPU
    (tests/test_spec_sample_cpu.py)."""
    from unimm_amd import lib as L
    from unimm_amd import lib as SP
    V, n, temp = 16, 65536, 0.7
    x1, xd1 = R.pair16()
    x = torch.from_numpy(x1).to(DEV)[None].repeat(n, 1)
    xd = torch.from_numpy(xd1).to(DEV)[None].repeat(n, 1)
    streams = torch.arange(n, dtype=torch.int32, device=DEV)
    t = torch.full((n,), temp, dtype=torch.float32, device=DEV)
    k = torch.zeros(n, dtype=torch.int32, device=DEV)
    p = torch.ones(n, dtype=torch.float32, device=DEV)
    d, acc, tok = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(3))
    f = [torch.empty(n, dtype=torch.float32, device=DEV) for _ in range(4)]
    L.lm_sample_rows(xd, n, V, None, None, SR.SEP, t, k, p, R.KEY_DRAFT, streams, d, f[0], f[1], f[2])
    SP.lm_spec_verify(x, xd, n, V, d, None, None, SR.SEP, t, k, p, R.KEY_ACCEPT, R.KEY_RESIDUAL, streams, acc, tok, *f)
    torch.cuda.synchronize()
    P, Q = R.softmax_kept(x1, temp), R.softmax_kept(xd1, temp)
    acc, tok, d = acc.cpu().numpy().astype(bool), tok.cpu().numpy(), d.cpu().numpy()
    assert (tok[acc] == d[acc]).all() and 0.2 < acc.mean() < 0.95
    stat, df = R.chi_square_cells(acc, tok, P, Q)
    crit = SR.chi_square_critical(df)
    macc, mtok, md = R.mirror_streams(x1, xd1, temp, np.arange(n))
    print(f"\nlm_spec_verify V = 16, {n} streams: chi^2 {stat:.2f} (df {df}, 0.1 % critical {crit:.2f}); acceptance {acc.mean():.4f}; "
          f"rows that differ from the float64 mirror: {(mtok != tok).sum()}")
    assert stat < crit
    assert (md != d).mean() < 1e-3 and (mtok != tok).mean() < 1e-3     # the mirror draws the same tokens up to fp32 near-ties
