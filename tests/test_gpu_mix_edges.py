"""unimm_lm_mix at its edges, through the C ABI, per element against tests/mix_ref.py: V in (3, 16, 257, 30522, 65536), rows in
(1, 3, 70), K = 1 .. 5, row strides V, V + 1 and a padded width, members of different strides with one base offset by a float
(the scalar path) and all-aligned members (the 16-byte path, with its V % 4 tail), both modes, the cut off / alpha = 0.1 / alpha
just below 1, banned ids inside and outside [0, V), every value of flags, -inf entries in PROB rows, NaN in every column at or
past V and in guard rows around every block, a sentinel around the output.

LOGIT and every cut decision are held bit for bit to the float32 restatement; PROB to the float64 definition within
4 x mix_ref.PROB_BUDGET = 2.52e-05 (the factor covers the device's expf / logf and fused products), with the -inf pattern equal.
Measured device maximum over every PROB launch of this file: 4.93e-06 (V = 65536, 70 rows, K = 2, the 16-byte path).

Further: planted rows (the maximum on a banned id; only sep and one id surviving), LOGIT (1, 0) and (0.5, 0.5) on two copies of a
row returning the row, every UNIMM_E_ARG case and rows = 0, and unimm_lm_mix chained into unimm_lm_topk."""
import numpy as np
import pytest
import torch

from tests import mix_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 2
SENT = -768.0
NEG = float("-inf")
BOUND = 4 * R.PROB_BUDGET
ALPHAS = (0.0, 0.1, float(np.nextafter(np.float32(1.0), np.float32(0.0))))
LAYOUTS = ("V", "V+1", "pad", "mixed")
worst = {"prob": 0.0}


def log_alpha(alpha):
    return float(np.float32(np.log(np.float64(alpha)))) if alpha > 0 else NEG


def pad_width(V):
    return (V + 63) // 64 * 64 + 64


def on_device(a, V, ld, shift=0):
    """rows of `a` inside NaN guard rows, NaN in the columns at or past V; shift = 1 moves the base off 16-byte alignment"""
    n = a.shape[0]
    flat = torch.full(((GUARD + n + GUARD) * ld + 4,), float("nan"), dtype=torch.float32)
    b = flat[shift:shift + (GUARD + n + GUARD) * ld].view(GUARD + n + GUARD, ld)
    b[GUARD:GUARD + n, :V] = torch.from_numpy(np.ascontiguousarray(a))
    flat = flat.to(DEV)
    return flat[shift:shift + (GUARD + n + GUARD) * ld].view(GUARD + n + GUARD, ld)[GUARD:GUARD + n]


def strides(layout, V, K):
    """(ld, shift) per member and of the output"""
    if layout == "mixed":
        pool = [(V, 0), (V + 1, 1), (pad_width(V), 0), (V + 3, 0), (pad_width(V), 1)]
        return pool[:K], (V + 1, 0)
    ld = {"V": V, "V+1": V + 1, "pad": pad_width(V)}[layout]
    return [(ld, 0)] * K, (ld, 0)


def launch(xs, weights, mode, V, layout, banned, flags, sep, la, rows=None):
    """One unimm_lm_mix launch -> the output rows on the host (fp32 [rows, V]); checks everything else stayed as it was."""
    from unimm_amd import mix as MX
    n, K = xs[0].shape[0], len(xs)
    rows = n if rows is None else rows
    lds, (ldo, so) = strides(layout, V, K)
    dx = [on_device(x, V, ld, sh) for x, (ld, sh) in zip(xs, lds)]
    flat = torch.full(((GUARD + n + GUARD) * ldo + 4,), SENT, dtype=torch.float32, device=DEV)
    whole = flat[so:so + (GUARD + n + GUARD) * ldo].view(GUARD + n + GUARD, ldo)
    out = whole[GUARD:GUARD + n]
    b = torch.tensor(banned, dtype=torch.int32, device=DEV) if banned is not None else None
    f = torch.tensor(flags, dtype=torch.int32, device=DEV) if flags is not None else None
    MX.lm_mix([d[:rows] for d in dx], weights, mode, V, b, f, sep, la, out[:rows])
    torch.cuda.synchronize()
    host = flat.cpu()
    got = host[so:so + (GUARD + n + GUARD) * ldo].view(GUARD + n + GUARD, ldo)
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[GUARD:GUARD + rows, :V] = False
    assert (got[keep] == SENT).all(), "wrote outside its rows or at / past column V"
    assert (host[:so] == SENT).all() and (host[so + (GUARD + n + GUARD) * ldo:] == SENT).all()
    res = got[GUARD:GUARD + rows, :V].numpy().copy()
    assert not np.isnan(res).any(), "read a column at or past V, or a row outside the launch"
    return res


def check(xs, weights, mode, V, layout, banned, flags, sep, la, what):
    got = launch(xs, weights, mode, V, layout, banned, flags, sep, la)
    cut = R.cut_mask(xs[0], banned, flags, sep, la)
    assert (got[cut] == NEG).all(), (what, "an id the cut removes is finite")
    if mode == R.LOGIT:
        want = R.mix_f32(xs, weights, mode, V, banned, flags, sep, la)
        bad = np.nonzero(got.view(np.int32) != want.view(np.int32))
        assert bad[0].size == 0, (what, bad[0][:4], bad[1][:4], got[bad][:4], want[bad][:4])
        return
    want = R.mix_f64(xs, weights, mode, V, banned, flags, sep, la)
    assert ((got == NEG) == (want == NEG)).all(), (what, "the -inf pattern differs")
    fin = np.isfinite(want)
    if fin.any():
        d = float(np.abs(got[fin].astype(np.float64) - want[fin]).max())
        worst["prob"] = max(worst["prob"], d)
        print(f"{what}: max |device - fp64| = {d:.3e} (bound {BOUND:.3e}; worst so far {worst['prob']:.3e})")
        assert d <= BOUND, what


def banned_ids(V):
    return [0, V - 1, -1, V, V + 5, 70000] + ([7, 101] if V > 102 else [])


def combos(V):
    if V < 1000:
        return [(rows, K) for rows in (1, 3, 70) for K in (1, 2, 3, 4, 5)]
    return [(1, 1), (3, 2), (3, 3), (1, 4), (3, 5), (70, 2)]


@pytest.mark.parametrize("mode", (R.LOGIT, R.PROB), ids=("logit", "prob"))
@pytest.mark.parametrize("V", (3, 16, 257, 30522, 65536))
def test_every_shape_layout_and_cut(V, mode):
    sep = 102 if V > 102 else 1
    n = 0
    for rows, K in combos(V):
        xs = R.edge_rows(V, rows, K, 1000 + V % 89 + 7 * rows + K, holes=mode == R.PROB, first=K % 2 == 0)
        weights = R.prob_weights(K) if mode == R.PROB else R.logit_weights(K)
        flags = [(r + K) % 4 for r in range(rows)]
        todo = [(LAYOUTS[(n + i) % 4], ALPHAS[(n + i) % 3]) for i in range(2)] if V >= 1000 else \
            [(lay, ALPHAS[(n + i) % 3]) for i, lay in enumerate(LAYOUTS)]
        for layout, alpha in todo:
            check(xs, weights, mode, V, layout, banned_ids(V), flags, sep, log_alpha(alpha),
                  f"V={V} rows={rows} K={K} {layout} alpha={alpha:.8g}")
        n += 1


@pytest.mark.parametrize("layout", ("pad", "mixed"))
@pytest.mark.parametrize("mode", (R.LOGIT, R.PROB), ids=("logit", "prob"))
def test_every_cut_on_every_layout(mode, layout):
    """V = 257 (one more than a multiple of 4: the 16-byte path has a tail), 3 rows, K = 3, every alpha with and without flags
    and banned ids"""
    V, K = 257, 3
    xs = R.edge_rows(V, 3, K, 5, holes=mode == R.PROB, first=True)
    weights = R.prob_weights(K) if mode == R.PROB else R.logit_weights(K)
    for alpha in ALPHAS:
        for banned, flags in ((None, None), (banned_ids(V), [1, 2, 3]), ([5], [0, 1, 0])):
            check(xs, weights, mode, V, layout, banned, flags, 102, log_alpha(alpha), f"{layout} alpha={alpha:.8g} {flags}")


@pytest.mark.parametrize("mode", (R.LOGIT, R.PROB), ids=("logit", "prob"))
def test_planted_rows(mode):
    """row 0: member 0's maximum is a banned id, so m0 is the best ELIGIBLE value and ids between the two survive; row 1: one id
    far above the rest, so only it and sep survive alpha = 0.1; row 2: the maximum is sep while flags ban it; row 3: the threshold
    met exactly (an id AT m0 + log_alpha stays, the next float below goes)."""
    V, sep, K = 257, 102, 2
    xs = R.edge_rows(V, 4, K, 21, scale=1.0, holes=False)
    la = log_alpha(0.1)
    x0 = xs[0]
    x0[0, 7] = x0[0].max() + 10.0
    x0[1] = -30.0
    x0[1, 40] = 5.0
    x0[2, sep] = x0[2].max() + 10.0
    x0[3] = -30.0
    x0[3, 9] = 4.0
    thr = np.float32(4.0) + np.float32(la)
    x0[3, 10], x0[3, 11] = thr, np.nextafter(thr, np.float32(NEG))
    banned, flags = [7], [0, 0, 1, 0]
    cut = R.cut_mask(x0, banned, flags, sep, la)
    assert not cut[0, 7] and 0 < cut[0].sum() < V - 2                       # the banned maximum is above the threshold: not cut
    assert sorted(np.nonzero(~cut[1])[0]) == [40, sep]
    assert not cut[2, sep] and cut[2].sum() < V - 1
    assert not cut[3, 10] and cut[3, 11] and sorted(np.nonzero(~cut[3])[0]) == [9, 10, sep]
    weights = [0.6, 0.4] if mode == R.PROB else [1.5, -0.5]
    for layout in ("pad", "mixed"):
        check(xs, weights, mode, V, layout, banned, flags, sep, la, f"planted {layout}")
        got = launch(xs, weights, mode, V, layout, banned, flags, sep, la)
        assert ((got == NEG) == cut).all()
    # every eligible id banned or flagged away: the row is not cut at all
    got = launch([x[:1, :3] for x in xs], weights, mode, 3, "V", [0, 2], [1], 1, la)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("V,layout", ((257, "pad"), (257, "mixed"), (30522, "pad")))
def test_logit_identities(V, layout):
    """(1, 0) and (0.5, 0.5) on two copies of a row return the row; K = 1 with weight 1 likewise"""
    x = R.edge_rows(V, 3, 1, 33, holes=False)[0]
    for weights, xs in (((1.0, 0.0), [x, x]), ((0.5, 0.5), [x, x]), ((1.0,), [x])):
        got = launch(xs, list(weights), R.LOGIT, V, layout, None, None, 102, NEG)
        assert (got.view(np.int32) == x.view(np.int32)).all(), weights


def test_prob_of_one_member_is_its_log_softmax():
    V = 30522
    x = R.edge_rows(V, 3, 2, 34, first=True)[1]
    got = launch([x], [1.0], R.PROB, V, "pad", None, None, 102, NEG)
    want = R.mix_f64([x], [1.0], R.PROB, V)
    fin = np.isfinite(want)
    assert ((got == NEG) == ~fin).all() and np.abs(got[fin] - want[fin]).max() <= BOUND


def test_fewer_rows_than_the_buffers_hold():
    xs = R.edge_rows(257, 5, 2, 35, holes=False)
    got = launch(xs, [0.5, 0.5], R.PROB, 257, "mixed", None, None, 102, log_alpha(0.1), rows=2)
    want = R.mix_f64([x[:2] for x in xs], [0.5, 0.5], R.PROB, 257, None, None, 102, log_alpha(0.1))
    fin = np.isfinite(want)
    assert ((got == NEG) == ~fin).all() and np.abs(got[fin] - want[fin]).max() <= BOUND


def test_refusals_and_no_rows():
    from unimm_amd import lib as L
    from unimm_amd import mix as MX
    V, rows = 16, 3
    x = [torch.randn(rows, V, device=DEV) for _ in range(6)]
    out = torch.full((rows, V), SENT, device=DEV)
    inf, nan = float("inf"), float("nan")
    ok = dict(rows_list=x[:2], weights=[0.5, 0.5], mode="prob", V=V, banned=None, flags=None, sep=1, log_alpha=NEG, out=out)
    bad = dict(
        no_members=dict(rows_list=[], weights=[]),
        six_members=dict(rows_list=x, weights=[1 / 6] * 6),
        wide=dict(V=65537),
        no_columns=dict(V=0),
        short_member=dict(rows_list=[x[0], torch.randn(rows, V - 1, device=DEV)]),
        short_out=dict(out=torch.empty(rows, V - 1, device=DEV)),
        mode=dict(mode=2), mode_name=dict(mode="mean"),
        nan_weight=dict(weights=[nan, 0.5]), inf_weight=dict(weights=[0.5, inf], mode="logit"),
        negative=dict(weights=[1.5, -0.5]), all_zero=dict(weights=[0.0, 0.0]),
        null_row=dict(rows_list=[x[0], None]), null_out=dict(out=None),
        same=dict(out=x[1]), overlap=dict(rows_list=[x[0], out.view(-1)[V // 2:V // 2 + 2 * V].view(2, V)], out=out[:2]),
    )
    for name, kw in bad.items():
        print(name)
        with pytest.raises(L.UnimmHipError, match="UNIMM_E_ARG"):
            MX.lm_mix(**{**ok, **kw})
    torch.cuda.synchronize()
    assert (out == SENT).all()
    MX.lm_mix(**{**ok, "weights": [1.5, -0.5], "mode": "logit"})              # a negative weight is LOGIT's to take
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == SENT).any()
    out.fill_(SENT)
    a = MX.LmMixArgs()                                                      # rows = 0 (an empty view has no address: by hand)
    a.K, a.mode, a.rows, a.V, a.ldo, a.sep, a.log_alpha = 2, MX.PROB, 0, V, V, 1, NEG
    for m in range(2):
        a.x[m], a.ld[m], a.w[m] = x[m].data_ptr(), V, 0.5
    a.out = out.data_ptr()
    MX._call("unimm_lm_mix", MX.C.byref(a))                                 # UNIMM_OK, nothing launched
    torch.cuda.synchronize()
    assert (out == SENT).all()


@pytest.mark.parametrize("mode", (R.LOGIT, R.PROB), ids=("logit", "prob"))
def test_chained_into_topk(mode):
    """unimm_lm_mix then unimm_lm_topk (K = 4) on the mixed rows, V = 30522, 70 rows, three members.  PROB: the row sums to 1, so
    topk's lse is 0 within the budget BOUND (measured: 9.5e-07) and its values are the float64 log-probabilities within 2 x BOUND
    (the row's own BOUND and the lse's).  Rank r of a row is DECIDED when the float64 values on both sides of it are more than
    BOUND apart; decided ranks carry the float64 id, and at most 2 % of the rows hold an undecided rank (these seeds: none, by the
    reference alone)."""
    from unimm_amd import lib as L
    from unimm_amd import mix as MX
    V, rows, K, top = 30522, 70, 3, 4
    xs = R.edge_rows(V, rows, K, 77, holes=False)
    weights = [0.5, 0.2, 0.3] if mode == R.PROB else [1.0, 0.5, -0.5]
    ld = pad_width(V)
    dx = [on_device(x, V, ld) for x in xs]
    mixed = torch.full((rows, ld), float("nan"), device=DEV)
    vals = torch.empty((rows, top), device=DEV)
    ids = torch.empty((rows, top), dtype=torch.int32, device=DEV)
    lse = torch.empty(rows, device=DEV)
    MX.lm_mix(dx, weights, mode, V, None, None, 102, NEG, mixed)
    L.lm_topk(mixed, rows, V, None, None, 102, top, vals, ids, lse)
    torch.cuda.synchronize()
    want = R.mix_f64(xs, weights, mode, V)
    order = np.argsort(-want, axis=1, kind="stable")[:, :top + 1]
    sv = np.take_along_axis(want, order, 1)
    gap = sv[:, :-1] - sv[:, 1:]                                            # gap[r]: between ranks r and r + 1
    tol = BOUND
    decided = (gap > tol) & np.concatenate([np.ones((rows, 1), bool), gap[:, :-1] > tol], 1)
    got = ids.cpu().numpy()
    assert (got[decided] == order[:, :top][decided]).all()
    undecided = float((~decided).any(1).mean())
    print(f"undecided rows: {undecided:.3f}")
    assert undecided <= 0.02
    if mode == R.PROB:
        worst_lse = float(lse.abs().max())
        print(f"max |lse| of a PROB row: {worst_lse:.3e}")
        assert worst_lse <= BOUND
        lp = np.take_along_axis(want, got.astype(np.int64), 1)
        assert np.abs(vals.cpu().numpy() - lp)[decided].max() <= 2 * BOUND
