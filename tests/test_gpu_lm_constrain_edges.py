"""unimm_lm_topk_hist / unimm_lm_sample_hist at their edges, by BIT EQUALITY against the existing entry points run one row at a
time on what tests/constrain_ref.py says the history rules make of the row -- so no tolerance is involved:

* penalty = 1: row i equals unimm_lm_sample_rows / unimm_lm_topk on that row with `banned` = the launch's list + the row's ban set;
* penalty != 1: token and logq (the top-1 id) equal the plain entry point's on the penalised row x', lse its lse on the raw row,
  logp (the top-1 value) the kernel's own fp32 expression x[token] - lse on the raw row;
* ngram = 0, penalty = 1: the launch equals the plain launch;
* permuting the rows permutes the results.

V = 257, 30522 and the three values around the history instantiation's staging bound (34816 is the last V it stages).  24 rows per
launch mix history lengths 0, n-2, n-1, n and ldh, periodic histories, rows with and without a context, a context with [SEP] and
ids outside [0, V), a length above ldh, negative lengths, context indices outside [0, nctx), flags 0 / 1 / 2 and a launch-wide
banned list."""
import functools

import numpy as np
import pytest
import torch

from tests import constrain_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEP = 102
ROWS, LDH, LDC, NCTX, KEY, K = 24, 16, 24, 4, 0x5EED1234, 4
VS = [257, 30522, 34815, 34816, 34817]
BANNED = [0, 101, 103, 7, 70000, -4]
SENT = -768.0


@functools.lru_cache(maxsize=2)
def logits(V):
    """-> (fp32 [ROWS, V] host rows, their device copy with three NaN columns past V): a few -inf, a few exact ties, one row of
    positive and one of negative logits only (the two branches of the penalty)."""
    g = torch.Generator().manual_seed(V)
    x = torch.randn((ROWS, V), generator=g) * 3.0
    x[:, 3:11] += 12.0                                                         # the histories' alphabet ranks high: bans matter
    x[:, 11] = x[:, 4]
    x[3, 5:9] = float("-inf")
    x[5] = x[5].abs() + 0.5
    x[6] = -x[6].abs() - 0.5
    x[7, 3:12] = 0.0
    xd = torch.full((ROWS, V + 3), float("nan"))
    xd[:, :V] = x
    return x.numpy(), xd.to(DEV)


def histories(V, n):
    """The launch's raw arrays (as the kernel gets them) for n-gram size n over the small alphabet 3 .. 10, where windows match."""
    rng = np.random.default_rng(1000 * n + V % 997)
    hist = rng.integers(3, 11, (ROWS, LDH)).astype(np.int32)
    hlen = rng.integers(0, LDH + 1, ROWS).astype(np.int32)
    for i, k in enumerate((0, max(n - 2, 0), max(n - 1, 0), n, LDH, LDH + 5, -1, min(n + 1, LDH))):
        hlen[i] = k
    hist[8] = np.resize([4, 9], LDH)                                           # a b a b a ...
    hist[9] = 6                                                                # a a a a ...
    hist[10] = np.resize([3, 4, 5], LDH)
    hlen[8:11] = (5, 4, 11)
    hist[11, :6] = (V + 1, 5, V + 1, 8, -3, V + 1)                             # ids outside [0, V) inside the windows
    hlen[11] = 6
    hist[12, :4] = (SEP, 5, SEP, 5)                                            # (a raw launch may hold [SEP]: it is never banned)
    hlen[12] = 4
    ctx = rng.integers(3, 11, (NCTX, LDC)).astype(np.int32)
    ctx[1, ::5] = SEP
    ctx[1, 3], ctx[1, 7], ctx[1, 8] = V + 5, -2, V
    ctx[2] = np.resize([4, 9, 9], LDC)
    clen = np.array([0, LDC - 5, LDC, LDC + 9], dtype=np.int32)                # context 0 is empty: a row without a context
    cidx = (np.arange(ROWS) % NCTX).astype(np.int32)
    cidx[20:] = (-3, NCTX, NCTX + 2, 0)                                        # clamp to 0, nctx - 1, nctx - 1
    hist[13:15] = np.resize([4, 9, 9], LDH)                                    # the period of context 2: long windows match
    hlen[13:15] = (LDH, 9)
    cidx[13:15] = 2
    return hist, hlen, ctx, clen, cidx


def sources(h, i, with_ctx=True):
    """Row i's sources as the header defines them from the raw arrays: every length and index clamped."""
    hist, hlen, ctx, clen, cidx = h
    a = hist[i, :min(max(int(hlen[i]), 0), LDH)].tolist()
    if not with_ctx:
        return a, None
    ci = min(max(int(cidx[i]), 0), NCTX - 1)
    return a, ctx[ci, :min(max(int(clen[ci]), 0), LDC)].tolist()


def row_params():
    i = np.arange(ROWS)
    return (np.array([1.0, 0.7, 2.0], dtype=np.float32)[i % 3], np.array([0, 1, 50, 5], dtype=np.int32)[i % 4],
            np.array([1.0, 0.9, 0.5, 1.0, 0.9], dtype=np.float32)[i % 5], (i % 3).astype(np.int32), (i * 7 + 1).astype(np.int32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def outputs(n, k=1):
    """Sentinel-filled outputs with one guard entry on either side."""
    tok = torch.full((n + 2,), -7, dtype=torch.int32, device=DEV)
    f = [torch.full((n + 2,), SENT, dtype=torch.float32, device=DEV) for _ in range(4)]
    vals = torch.full((n + 2, k), SENT, dtype=torch.float32, device=DEV)
    ids = torch.full((n + 2, k), -7, dtype=torch.int32, device=DEV)
    return tok, f[0], f[1], f[2], vals, ids, f[3]


def collect(out, n):
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in out]
    for o in host:
        assert (o[0] == (-7 if o.dtype == np.int32 else SENT)).all() and (o[n + 1] == (-7 if o.dtype == np.int32 else SENT)).all()
    return dict(zip(("tok", "lp", "lq", "lse", "vals", "ids", "tlse"), (o[1:n + 1] for o in host)))


def hist_launch(V, h, n, r, k=K, order=None, with_ctx=True):
    """One launch of each _hist entry point on all rows (in `order`) -> host results, and the struct's fp32 inv_penalty."""
    from unimm_amd import lib as L
    order = np.arange(ROWS) if order is None else order
    _, xd = logits(V)
    t, tk, tp, flags, streams = (dev(a[order]) for a in row_params())
    hist, hlen, ctx, clen, cidx = h
    args = [dev(hist[order]), dev(hlen[order])] + ([dev(ctx), dev(clen), dev(cidx[order])] if with_ctx else [None] * 3)
    hs = L.lm_history(args[0], args[1], n, r, SEP, *args[2:])
    assert (hs.ldh, hs.ldc, hs.nctx) == (LDH, LDC if with_ctx else 0, NCTX if with_ctx else 0)
    x = xd[dev(order).long()]
    banned = dev(np.array(BANNED, dtype=np.int32))
    out = outputs(ROWS, k)
    body = slice(1, ROWS + 1)
    L.lm_sample_hist(x, ROWS, V, banned, flags, SEP, t, tk, tp, KEY, streams, hs, out[0][body], out[1][body], out[2][body], out[3][body])
    L.lm_topk_hist(x, ROWS, V, banned, flags, SEP, k, hs, out[4][body], out[5][body], out[6][body])
    return collect(out, ROWS), np.float32(hs.inv_penalty)


def plain_rows(V, rows_x, ban_sets, k=K):
    """The existing entry points, one launch per row: row i of `rows_x` (device fp32 [ROWS, >= V]) with banned = the launch's
    list + ban_sets[i]."""
    from unimm_amd import lib as L
    t, tk, tp, flags, streams = (dev(a) for a in row_params())
    out = outputs(ROWS, k)
    keep = []
    for i in range(ROWS):
        b = dev(np.array(BANNED + sorted(ban_sets[i]), dtype=np.int32))
        keep.append(b)
        s = slice(i + 1, i + 2)
        L.lm_sample_rows(rows_x[i:i + 1], 1, V, b, flags[i:i + 1], SEP, t[i:i + 1], tk[i:i + 1], tp[i:i + 1], KEY, streams[i:i + 1],
                         out[0][s], out[1][s], out[2][s], out[3][s])
        L.lm_topk(rows_x[i:i + 1], 1, V, b, flags[i:i + 1], SEP, k, out[4][s], out[5][s], out[6][s])
    return collect(out, ROWS)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("V", VS)
def test_ngram_bans_equal_the_plain_entry_points_with_the_ban_set(V):
    _, xd = logits(V)
    for n in (1, 2, 3, 8):
        for with_ctx in (True, False):
            if not with_ctx and n in (3, 8):
                continue
            h = histories(V, n)
            bans = [CR.ban_set(*sources(h, i, with_ctx), n, V, SEP) for i in range(ROWS)]
            assert sum(bool(b) for b in bans) >= {1: 12, 2: 8, 3: 4, 8: 2}[n], "the rule has work to do"
            got, _ = hist_launch(V, h, n, 1.0, with_ctx=with_ctx)
            want = plain_rows(V, xd, bans)
            for f in ("tok", "lp", "lq", "lse", "vals", "ids", "tlse"):
                assert same_bits(got[f], want[f]), (V, n, with_ctx, f, np.nonzero(got[f] != want[f]))
            free = plain_rows(V, xd, [set()] * ROWS)
            assert (free["ids"] != got["ids"]).any() or n > 2                  # and it changes the first ids of the order
            assert (got["tok"] >= 0).sum() >= ROWS - 2 and not np.isnan(got["lp"]).any() and not np.isnan(got["lq"]).any()


@pytest.mark.parametrize("V", VS)
def test_penalty_selects_on_the_penalised_row_and_reports_the_raw_log_p(V):
    x, xd = logits(V)
    moved = 0
    for n, r in ((0, 2.0), (2, 0.5), (3, 1.7)):
        h = histories(V, max(n, 1))
        got, inv = hist_launch(V, h, n, r, k=1)
        assert same_bits(inv, np.float32(1.0 / float(np.float32(r))))
        bans = [CR.ban_set(*sources(h, i), n, V, SEP) for i in range(ROWS)]
        xp = np.stack([CR.penalised_row(x[i], *sources(h, i), np.float32(r), inv) for i in range(ROWS)])
        assert (xp != x).sum() >= ROWS
        pen = plain_rows(V, dev(xp), bans, k=1)
        raw = plain_rows(V, xd, bans, k=1)
        assert same_bits(got["tok"], pen["tok"]) and same_bits(got["lq"], pen["lq"]), (V, n, r)
        assert same_bits(got["lse"], raw["lse"]) and same_bits(got["tlse"], raw["tlse"]) and same_bits(got["lse"], got["tlse"])
        assert same_bits(got["ids"], pen["ids"])
        drawn = got["tok"] >= 0
        assert drawn.sum() >= ROWS - 2
        with np.errstate(invalid="ignore"):
            lp = np.where(drawn, x[np.arange(ROWS), np.maximum(got["tok"], 0)] - got["lse"], np.float32("-inf")).astype(np.float32)
            top = got["ids"][:, 0]
            val = np.where(pen["vals"][:, 0] > -np.inf, x[np.arange(ROWS), top] - got["lse"], np.float32("-inf")).astype(np.float32)
        assert same_bits(got["lp"], lp) and same_bits(got["vals"][:, 0], val), (V, n, r)
        moved += int((got["ids"] != raw["ids"]).sum())
        assert (got["lq"] != raw["lq"]).any()                                   # the penalty matters ...
        sampled = drawn & (row_params()[1] != 1) & (row_params()[3] != 2)
        assert (got["lq"][sampled] != got["lp"][sampled]).any() and np.isfinite(got["lq"][drawn]).all()
    assert moved > 0                                                           # ... to the first id of the order too


@pytest.mark.parametrize("V", VS)
def test_no_rule_is_the_plain_launch(V):
    from unimm_amd import lib as L
    _, xd = logits(V)
    got, _ = hist_launch(V, histories(V, 2), 0, 1.0)
    t, tk, tp, flags, streams = (dev(a) for a in row_params())
    banned = dev(np.array(BANNED, dtype=np.int32))
    out = outputs(ROWS, K)
    body = slice(1, ROWS + 1)
    L.lm_sample_rows(xd, ROWS, V, banned, flags, SEP, t, tk, tp, KEY, streams, out[0][body], out[1][body], out[2][body], out[3][body])
    L.lm_topk(xd, ROWS, V, banned, flags, SEP, K, out[4][body], out[5][body], out[6][body])
    want = collect(out, ROWS)
    for f in want:
        assert same_bits(got[f], want[f]), (V, f)
    # ... and so is a launch without a history at all
    hs = L.lm_history(None, None, 0, 1.0, SEP)
    out = outputs(ROWS, K)
    L.lm_sample_hist(xd, ROWS, V, banned, flags, SEP, t, tk, tp, KEY, streams, hs, out[0][body], out[1][body], out[2][body], out[3][body])
    L.lm_topk_hist(xd, ROWS, V, banned, flags, SEP, K, hs, out[4][body], out[5][body], out[6][body])
    none = collect(out, ROWS)
    for f in want:
        assert same_bits(none[f], want[f]), (V, f)


@pytest.mark.parametrize("V", [257, 34816, 34817])
def test_a_row_depends_on_its_own_data_alone(V):
    perm = np.random.default_rng(V).permutation(ROWS)
    for n, r in ((2, 1.0), (3, 1.3)):
        h = histories(V, n)
        a, _ = hist_launch(V, h, n, r)
        b, _ = hist_launch(V, h, n, r, order=perm)
        c, _ = hist_launch(V, h, n, r)
        for f in a:
            assert same_bits(a[f][perm], b[f]) and same_bits(a[f], c[f]), (V, n, r, f)


def test_refused_launches_write_nothing():
    from unimm_amd import lib as L
    V = 257
    _, xd = logits(V)
    t, tk, tp, flags, streams = (dev(a) for a in row_params())
    hist, hlen, _, _, _ = (dev(a) for a in histories(V, 2))
    out = outputs(ROWS, K)
    body = slice(1, ROWS + 1)
    for n, r, hh in ((9, 1.0, hist), (-1, 1.0, hist), (2, 0.0, hist), (2, float("nan"), hist), (2, float("inf"), hist), (2, 1.0, None),
                     (0, 1.3, None)):
        hs = L.lm_history(hh, hlen if hh is not None else None, n, r if r == r and 0 < r < float("inf") else 1.0, SEP)
        hs.penalty = r
        with pytest.raises(L.UnimmHipError, match="UNIMM_E_"):
            L.lm_sample_hist(xd, ROWS, V, None, flags, SEP, t, tk, tp, KEY, streams, hs, out[0][body], out[1][body], out[2][body], out[3][body])
        with pytest.raises(L.UnimmHipError, match="UNIMM_E_"):
            L.lm_topk_hist(xd, ROWS, V, None, flags, SEP, K, hs, out[4][body], out[5][body], out[6][body])
    torch.cuda.synchronize()
    for o in out:
        assert (o == (-7 if o.dtype == torch.int32 else SENT)).all()
