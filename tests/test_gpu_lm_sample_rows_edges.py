"""unimm_lm_sample_rows (per-row temperature / top_k / top_p) at its edges: V in (1, 257, 30522, 36865) -- one id, a block edge,
the production vocabulary on the LDS-staged path and the first size past it on the re-read path -- with every row's parameters
drawn from SR.TEMPS x top_k in (0, 1, 2, V, V + 5) x top_p in (1, 0.9, 1e-6), mixed within each launch (all 45 combinations occur
for every V).  The cases and the checker are those of tests/sample_ref.py; V = 1 is below what its planted rows need, so that
case is built here (every flag, +-0, -inf, large offsets).

(a) every row is bit-identical (token, logp, logq, lse) to the scalar unimm_lm_sample launched on that row alone with that row's
    parameters -- an equality, the arithmetic is the same; the scalar kernel is pinned against the float64 restatement by
    tests/test_gpu_generate_sample_edges.py, and the rows are put through SR.check_rows here as well;
(b) top_k = 1 rows return the first id and value of unimm_lm_topk(K = 1) bit for bit and logq == 0 (exact ties, +-0 included);
(c) a row does not depend on the other rows' parameters, and a launch repeats bit for bit;
(d) rows with invalid parameters, all -inf rows, the two flags, NaN past V and around the rows, NULL arrays and rows = 0.

Every launch runs on guarded, sentinel-filled buffers as in tests/test_gpu_generate_sample_edges.py."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from oracle import generate_ref as GR
from tests import sample_ref as SR

pytestmark = pytest.mark.gpu
GUARD = GR.GUARD
SENT = -768.0
DEV = "cuda"
KEY = SR.CASE_KEY
VS = (1, 257, 30522, 36865)
TOP_PS = (1.0, 0.9, 1e-6)


def top_ks(V):
    return (0, 1, 2, V, V + 5)


def combos(V):
    return list(itertools.product(SR.TEMPS, top_ks(V), TOP_PS))       # 45 of (temperature, top_k, top_p)


def row_params(V, n, launch_no):
    """Parameters of the n rows of launch `launch_no`: row r takes combination 11 (r + launch_no n) mod 45 (11 and 45 are coprime:
    45 consecutive rows see all 45) -> (fp32 [n], int32 [n], fp32 [n])."""
    cs = combos(V)
    pick = [cs[(11 * (r + launch_no * n)) % len(cs)] for r in range(n)]
    return (torch.tensor([c[0] for c in pick], dtype=torch.float32), torch.tensor([c[1] for c in pick], dtype=torch.int32),
            torch.tensor([c[2] for c in pick], dtype=torch.float32))


def launches(V, n):
    return max(2, -(-len(combos(V)) // n))


def one_id_case():
    """V = 1: the id is eligible, banned by a flag (sep = 102 is not in the row: SEP_FORCED leaves nothing), or -inf."""
    xs = [0.5, -0.0, 0.0, -math.inf, 1e4, -1e4, -3.0, 2.0, 7.5, -math.inf, 1.0, -2.5, 3e-39, -0.25, 40.0]
    flags = [0, 0, 1, 0, 0, 1, 2, 3, 0, 2, 1, 0, 0, 1, 0]
    n = len(xs)
    return dict(x=torch.tensor(xs, dtype=torch.float32).view(n, 1), flags=torch.tensor(flags, dtype=torch.int32),
                banned=torch.tensor([7, -1, 1], dtype=torch.int32), streams=torch.arange(n, dtype=torch.int32) * 31 - 4,
                names=["one id %d" % r for r in range(n)], V=1)


@functools.lru_cache(maxsize=None)
def case_and_rows(V):
    case = one_id_case() if V == 1 else SR.sample_case(V)
    return case, SR.case_rows(case)


class Buffers:
    """The case on the device: logits inside NaN guard rows with padded columns, and what the scalar kernel gives per row."""

    def __init__(self, V, ld=None, pad=float("nan")):
        case, self.rows = case_and_rows(V)
        self.case, self.V = case, V
        self.n = n = case["x"].shape[0]
        self.ld = ld = (V + 63) // 64 * 64 + 64 if ld is None else ld
        xb = torch.full((GUARD + n + GUARD, ld), float("nan"), dtype=torch.float32)
        xb[GUARD:GUARD + n, V:] = pad
        xb[GUARD:GUARD + n, :V] = case["x"]
        self.x = xb.to(DEV)[GUARD:GUARD + n]
        self.banned, self.flags, self.streams = (case[k].to(DEV) for k in ("banned", "flags", "streams"))

    def outputs(self):
        N = GUARD + self.n + GUARD
        tok = torch.full((N,), -7, dtype=torch.int32, device=DEV)
        return (tok,) + tuple(torch.full((N,), SENT, dtype=torch.float32, device=DEV) for _ in range(3))

    def finish(self, outs, rows=None, want_lse=True):
        """-> (token, logp, logq, lse) host arrays of the written rows, after checking that nothing else was written."""
        torch.cuda.synchronize()
        rows = self.n if rows is None else rows
        tok, lp, lq, lse = (o.cpu() for o in outs)
        keep = torch.ones(tok.shape[0], dtype=torch.bool)
        keep[GUARD:GUARD + rows] = False
        assert (tok[keep] == -7).all() and (lp[keep] == SENT).all() and (lq[keep] == SENT).all(), "wrote outside its rows"
        assert (lse[keep] == SENT).all() and (want_lse or (lse == SENT).all()), "wrote lse outside its rows"
        body = slice(GUARD, GUARD + rows)
        assert not torch.isnan(lp[body]).any() and not torch.isnan(lq[body]).any()
        return tok[body].numpy(), lp[body].numpy(), lq[body].numpy(), lse[body].numpy()

    def per_row(self, params, key=KEY, rows=None, want_lse=True):
        """One unimm_lm_sample_rows launch."""
        from unimm_amd import lib as L
        outs = self.outputs()
        b = slice(GUARD, GUARD + self.n)
        t, k, p = (a.to(DEV) for a in params)
        L.lm_sample_rows(self.x, self.n if rows is None else rows, self.V, self.banned, self.flags, SR.SEP, t, k, p, key, self.streams,
                         outs[0][b], outs[1][b], outs[2][b], outs[3][b] if want_lse else None)
        return self.finish(outs, rows, want_lse)

    def scalar(self, params, key=KEY):
        """unimm_lm_sample launched once per row, on that row alone, with that row's parameters."""
        from unimm_amd import lib as L
        outs = self.outputs()
        for r in range(self.n):
            o = slice(GUARD + r, GUARD + r + 1)
            L.lm_sample(self.x[r:r + 1], 1, self.V, self.banned, self.flags[r:r + 1], SR.SEP, float(params[0][r]), int(params[1][r]),
                        float(params[2][r]), key, self.streams[r:r + 1], outs[0][o], outs[1][o], outs[2][o], outs[3][o])
        return self.finish(outs)

    def topk1(self):
        from unimm_amd import lib as L
        vals = torch.empty((self.n, 1), dtype=torch.float32, device=DEV)
        ids = torch.empty((self.n, 1), dtype=torch.int32, device=DEV)
        L.lm_topk(self.x, self.n, self.V, self.banned, self.flags, SR.SEP, 1, vals, ids)
        torch.cuda.synchronize()
        return vals.cpu().numpy()[:, 0], ids.cpu().numpy()[:, 0]


def bits(a):
    return a.view(np.int32)


def assert_same(got, want, rows=None, what=""):
    for name, g, w in zip(("token", "logp", "logq", "lse"), got, want):
        g, w = (bits(g), bits(w)) if rows is None else (bits(g)[rows], bits(w)[rows])
        assert np.array_equal(g, w), (what, name, np.nonzero(g != w)[0][:8])


@pytest.mark.parametrize("V", VS)
def test_rows_equal_the_scalar_kernel_bit_for_bit(V):
    b = Buffers(V)
    seen = set()
    draws = undecided = 0
    for no in range(launches(V, b.n)):
        params = row_params(V, b.n, no)
        got = b.per_row(params)
        assert_same(got, b.scalar(params), what=f"V {V} launch {no}")
        # the float64 restatement, per group of rows that share their parameters
        groups = {}
        for r in range(b.n):
            groups.setdefault((float(params[0][r]), int(params[1][r]), float(params[2][r])), []).append(r)
        for (t, k, p), idx in groups.items():
            d, u, _ = SR.check_rows([b.rows[r] for r in idx], V, t, k, p, *(a[idx] for a in got), what=f"V {V} rows {idx[:4]} ({t}, {k}, {p})")
            draws, undecided = draws + d, undecided + u
        seen |= set(groups)
    print(f"\nlm_sample_rows V = {V}: {undecided} of {draws} draws undecided in the float64 restatement")
    want = {(float(torch.tensor(t, dtype=torch.float32)), k, float(torch.tensor(p, dtype=torch.float32))) for t, k, p in combos(V)}
    assert seen == want and len(want) == (45 if V > 2 else 36) and draws > 0   # (V = 1: top_k = V is top_k = 1 again)


@pytest.mark.parametrize("V", VS)
def test_top_k_1_rows_are_lm_topk(V):
    b = Buffers(V, ld=V)
    vals, ids = b.topk1()
    n = b.n
    mixed = row_params(V, n, 0)
    # every row greedy, under every temperature / top_p of the suite in turn; then only the top_k = 1 rows of a mixed launch
    ts = torch.tensor([SR.TEMPS[r % 3] for r in range(n)], dtype=torch.float32)
    ps = torch.tensor([TOP_PS[(r // 3) % 3] for r in range(n)], dtype=torch.float32)
    for params, sel in ((mixed, mixed[1].numpy() == 1), ((ts, torch.ones(n, dtype=torch.int32), ps), np.ones(n, dtype=bool))):
        tok, lp, lq, _ = b.per_row(params)
        some = sel & (tok >= 0)
        assert sel.sum() > 0 and (V == 1 or some.sum() >= sel.sum() - 8)
        assert np.array_equal(tok[some], ids[some])
        assert np.array_equal(bits(lp[some]), bits(vals[some])), np.nonzero(bits(lp) != bits(vals))[0][:8]
        assert (lq[some] == 0.0).all()
        none = sel & (tok < 0)                                         # nothing eligible: lm_topk's best is banned or -inf
        assert not (vals[none] > -np.inf).any() and (lp[none] == -np.inf).all() and (lq[none] == -np.inf).all()
    if V > 1:                                                          # (every row greedy) planted ties go to the smaller id, +-0 tie
        names = b.case["names"]
        for name in ("all equal", "plateau on top", "signed zeros", "ties across lanes 63/64 and threads 255/256"):
            r = names.index(name)
            assert tok[r] == ids[r] == b.rows[r].ids[0], (name, tok[r], ids[r])


@pytest.mark.parametrize("V", VS)
def test_other_rows_parameters_do_not_matter_and_launches_repeat(V):
    b = Buffers(V, ld=V + 3, pad=1e30)
    n = b.n
    params = row_params(V, n, 1)
    a = b.per_row(params)
    assert_same(b.per_row(params), a, what="repeated launch")
    nolse = b.per_row(params, want_lse=False)
    assert_same(nolse[:3], a[:3], what="without lse")
    fixed = np.arange(n) % 4 == 0                                      # these keep their parameters; the others trade theirs
    others = np.nonzero(~fixed)[0]
    perm = np.arange(n)
    perm[others] = np.roll(others, 5)
    moved = tuple(p[torch.from_numpy(perm)] for p in params)
    assert any((m[others] != p[others]).any() for m, p in zip(moved, params))
    c = b.per_row(moved)
    assert_same(c, a, rows=fixed, what="other rows' parameters permuted")
    assert_same(c, b.scalar(moved), what="the rows that took another row's parameters")
    if V > 1:
        assert (c[0][others] != a[0][others]).any()                    # the parameters matter
        other = b.per_row(params, key=KEY + 1)[0]
        assert (other != a[0]).any()                                   # and so does the key


INVALID = [(0.0, 0, 1.0), (-1.0, 0, 1.0), (float("nan"), 0, 1.0), (float("inf"), 0, 1.0), (-float("inf"), 1, 1.0), (-0.0, 0, 0.5),
           (1.0, 0, 0.0), (1.0, 0, 1.5), (1.0, 0, float("nan")), (1.0, 2, -0.1), (1.0, 0, 1.0000001), (1.0, -1, 1.0),
           (0.7, -2 ** 31, 0.9), (float("nan"), -5, float("nan"))]


@pytest.mark.parametrize("V", VS)
def test_invalid_rows_and_special_rows(V):
    b = Buffers(V)
    n = b.n
    params = row_params(V, n, 0)
    good = b.per_row(params)
    t, k, p = (a.clone() for a in params)
    bad = np.zeros(n, dtype=bool)
    for i, (ti, ki, pi) in enumerate(INVALID):
        r = (4 * i + 1) % n                                            # spread over the rows, planted ones included
        t[r], k[r], p[r] = ti, ki, pi
        bad[r] = True
    assert bad.sum() == len(INVALID)
    got = b.per_row((t, k, p))
    assert (got[0][bad] == -1).all() and (got[1][bad] == -np.inf).all() and (got[2][bad] == -np.inf).all()
    assert np.array_equal(bits(got[3]), bits(good[3]))                 # lse is written for every row, invalid or not
    assert_same(got, good, rows=~bad, what="rows next to invalid ones")
    # nothing eligible (all -inf, everything banned, a flag that leaves nothing): the defined result, lse as the restatement has it
    empty = np.array([r.n == 0 for r in b.rows])
    assert empty.sum() >= 3
    assert (good[0][empty] == -1).all() and (good[1][empty] == -np.inf).all() and (good[2][empty] == -np.inf).all()
    for r in np.nonzero(empty)[0]:
        want = b.rows[r].lse
        assert good[3][r] == want if not math.isfinite(want) else abs(good[3][r] - want) <= 1e-3 * max(1.0, abs(want))
    assert (good[0][~empty] >= 0).all() and (good[0] < V).all()
    # the flags: SEP_FORCED with a finite [SEP] logit returns [SEP] with logq = 0 whatever the row's parameters are, SEP_BANNED
    # never returns it
    flags = b.case["flags"].numpy()
    forced, sep_banned = (flags & 2) != 0, (flags & 1) != 0
    assert (good[0][sep_banned] != SR.SEP).all()
    if V > SR.SEP:
        live = forced & ~empty
        assert live.sum() >= 1 and (good[0][live] == SR.SEP).all() and (good[2][live] == 0.0).all()
        for no in range(1, 4):
            again = b.per_row(row_params(V, n, no))
            assert (again[0][live] == SR.SEP).all() and (again[2][live] == 0.0).all()
            assert np.array_equal(bits(again[1][live]), bits(good[1][live]))


def test_null_arrays_and_zero_rows():
    from unimm_amd import lib as L
    V = 257
    b = Buffers(V)
    n = b.n
    t, k, p = (a.to(DEV) for a in row_params(V, n, 0))
    tok = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lp, lq, lse = (torch.full((n,), SENT, dtype=torch.float32, device=DEV) for _ in range(3))
    for args in ((None, k, p), (t, None, p), (t, k, None), (None, None, None)):
        with pytest.raises(L.UnimmHipError, match="UNIMM_E_ARG"):
            L.lm_sample_rows(b.x, n, V, None, None, SR.SEP, *args, KEY, b.streams, tok, lp, lq, lse)
    with pytest.raises(L.UnimmHipError, match="UNIMM_E_ARG"):
        L.lm_sample_rows(b.x, n, V, None, None, SR.SEP, t, k, p, KEY, None, tok, lp, lq, lse)
    L.lm_sample_rows(b.x, 0, V, None, None, SR.SEP, t, k, p, KEY, b.streams, tok, lp, lq, lse)
    torch.cuda.synchronize()
    assert (tok == -7).all() and (lp == SENT).all() and (lq == SENT).all() and (lse == SENT).all()
    assert b.per_row((t, k, p), rows=0)[0].size == 0
    part = b.per_row((t, k, p), rows=5)                                # fewer rows than the buffers hold: the rest keeps its sentinels
    assert_same(part, tuple(a[:5] for a in b.per_row((t, k, p))))
