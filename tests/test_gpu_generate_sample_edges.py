"""unimm_lm_sample per element at every edge, against the float64 restatement of tests/sample_ref.py (its budgets and their
measured constants are derived there): V in (16, 255, 256, 257, 1000, 30522, 65536) x top_k in (0, 1, 2, 50, V) x top_p in
(1, 0.9, 0.5, 1e-6) x temperature in (1, 0.7, 2), 64 planted and random rows per case, and one V = 16 case of 4,096 rows that
share one logits row and differ in their stream.

Every launch runs on buffers with NaN guard rows before and after the logits and columns past V that hold NaN or 1e30 (never
read); the outputs are pre-filled with sentinels that everything outside the `rows` written entries must keep.  A decided draw
(float64 top-2 gap of the perturbed values above E_draw) must be the float64 argmax, an undecided one an id within E_draw of the
best; at most 0.1 % of a test's draws may be undecided -- a condition on the inputs, checked on the CPU as well."""
import functools

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


def launch(x, V, ld, banned, flags, streams, t, k, p, key=KEY, rows=None, pad=float("nan"), want_lse=True):
    """-> (token, logp, logq, lse) host arrays of the `rows` written entries, from guarded, sentinel-filled outputs."""
    from unimm_amd import lib as L
    n = x.shape[0]
    rows = n if rows is None else rows
    xb = torch.full((GUARD + n + GUARD, ld), float("nan"), dtype=torch.float32)
    xb[GUARD:GUARD + n, V:] = pad
    xb[GUARD:GUARD + n, :V] = x
    xd = xb.to(DEV)
    N = GUARD + n + GUARD
    tok = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    lp, lq, lse = (torch.full((N,), SENT, dtype=torch.float32, device=DEV) for _ in range(3))
    body = slice(GUARD, GUARD + n)
    L.lm_sample(xd[body], rows, V, None if banned is None else banned.to(DEV), None if flags is None else flags.to(DEV), SR.SEP,
                t, k, p, key, streams.to(DEV), tok[body], lp[body], lq[body], lse[body] if want_lse else None)
    torch.cuda.synchronize()
    tok, lp, lq, lse = tok.cpu(), lp.cpu(), lq.cpu(), lse.cpu()
    keep = torch.ones(N, dtype=torch.bool)
    keep[GUARD:GUARD + rows] = False
    assert (tok[keep] == -7).all() and (lp[keep] == SENT).all() and (lq[keep] == SENT).all(), "lm_sample wrote outside its rows"
    assert (lse[keep] == SENT).all() and (want_lse or (lse == SENT).all()), "lm_sample wrote lse outside its rows"
    body = slice(GUARD, GUARD + rows)
    assert not torch.isnan(lp[body]).any() and not torch.isnan(lq[body]).any()
    return tok[body].numpy(), lp[body].numpy(), lq[body].numpy(), lse[body].numpy()


@functools.lru_cache(maxsize=2)
def case_and_rows(V):
    case = SR.sample_case(V)
    return case, SR.case_rows(case)


@pytest.mark.parametrize("temperature", SR.TEMPS)
@pytest.mark.parametrize("V", SR.SAMPLE_V)
def test_lm_sample_edges(V, temperature):
    case, rows = case_and_rows(V)
    x, banned, flags, streams = case["x"], case["banned"], case["flags"], case["streams"]
    draws = undecided = 0
    worst = np.zeros(3)
    for i, k in enumerate(SR.top_ks(V)):
        for j, p in enumerate(SR.TOP_PS):
            ld, pad = ((V + 63) // 64 * 64 + 64, float("nan")) if (i + j) % 3 == 0 else (V + 1, 1e30) if (i + j) % 3 == 1 else (V, 0.0)
            what = f"V {V} top_k {k} top_p {p} temperature {temperature} ldl {ld}"
            tok, lp, lq, lse = launch(x, V, ld, banned, flags, streams, temperature, k, p)
            d, u, w = SR.check_rows(rows, V, temperature, k, p, tok, lp, lq, lse, what=what)
            draws, undecided, worst = draws + d, undecided + u, np.maximum(worst, w)
    print(f"\nlm_sample V = {V}, temperature {temperature}: {undecided} of {draws} draws undecided; worst |err| / E: lse {worst[0]:.3f}, "
          f"logp {worst[1]:.3f}, logq {worst[2]:.3f}")
    assert draws > 0 and undecided <= 1e-3 * draws


@pytest.mark.parametrize("V", SR.SAMPLE_V)
def test_top_k_1_is_lm_topk_first_id(V):
    from unimm_amd import lib as L
    case, _ = case_and_rows(V)
    x, banned, flags = case["x"].to(DEV), case["banned"].to(DEV), case["flags"].to(DEV)
    n = x.shape[0]
    vals = torch.empty((n, 1), dtype=torch.float32, device=DEV)
    ids = torch.empty((n, 1), dtype=torch.int32, device=DEV)
    L.lm_topk(x, n, V, banned, flags, SR.SEP, 1, vals, ids)
    for t, p in ((1.0, 1.0), (0.7, 0.5)):
        tok, lp, lq, _ = launch(case["x"], V, V, case["banned"], case["flags"], case["streams"], t, 1, p)
        some = tok >= 0
        v = vals.cpu().numpy()[:, 0]
        assert some.sum() >= n - 8
        assert (tok[some] == ids.cpu().numpy()[some, 0]).all()
        assert not (v[~some] > -np.inf).any()                                  # nothing eligible: lm_topk's best is a banned id
        assert np.allclose(lp[some], v[some], rtol=1e-6, atol=1e-5) and (lq[some] == 0.0).all()


@pytest.mark.parametrize("V", [257, 30522, 65536])
def test_rows_are_independent_and_launches_repeat(V):
    """Permuting the rows together with their flags and streams permutes the outputs bit for bit; a second launch with the same
    arguments is bit-identical; without lse nothing is written to it."""
    case, _ = case_and_rows(V)
    x, banned, flags, streams = case["x"], case["banned"], case["flags"], case["streams"]
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(V))
    for k, p, t in ((0, 1.0, 1.0), (50, 0.9, 0.7), (0, 0.5, 2.0)):
        a = launch(x, V, V, banned, flags, streams, t, k, p)
        b = launch(x, V, V, banned, flags, streams, t, k, p)
        c = launch(x[perm], V, V + 3, banned, flags[perm], streams[perm], t, k, p)
        d = launch(x, V, V, banned, flags, streams, t, k, p, want_lse=False)
        for u, v, w, z in zip(a, b, c, d[:3] + (a[3],)):
            assert np.array_equal(u.view(np.int32), v.view(np.int32))
            assert np.array_equal(u[perm.numpy()].view(np.int32), w.view(np.int32))
            assert np.array_equal(u.view(np.int32), z.view(np.int32))
        other = launch(x, V, V, banned, flags, streams + 1, t, k, p)[0]
        assert (other != a[0]).any()                                           # the stream matters


def test_4096_rows_share_one_logits_row():
    V, n = 16, 4096
    x = (torch.randn(V, generator=torch.Generator().manual_seed(0)) * 1.5).repeat(n, 1)
    streams = torch.arange(n, dtype=torch.int32)
    banned = torch.tensor([0], dtype=torch.int32)
    rows = [SR.Row(x[0].numpy(), V, banned, 0, SR.SEP, KEY, s) for s in range(n)]
    for k, p, t in ((0, 1.0, 1.0), (5, 0.9, 0.7)):
        tok, lp, lq, lse = launch(x, V, V, banned, None, streams, t, k, p)
        draws, undecided, _ = SR.check_rows(rows, V, t, k, p, tok, lp, lq, lse, what=f"4096 rows top_k {k}")
        assert draws == n and undecided <= 1e-3 * n
        assert len(set(tok.tolist())) > 3
        assert (lse == lse[0]).all()


def test_refusals_and_zero_rows():
    """temperature <= 0 (or not finite), top_p outside (0, 1] and top_k < 0 return UNIMM_E_ARG before any launch; rows = 0 returns
    OK without one: the outputs keep their sentinels either way."""
    from unimm_amd import lib as L
    V = 257
    case, _ = case_and_rows(V)
    x, streams = case["x"].to(DEV), case["streams"].to(DEV)
    n = x.shape[0]
    tok = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lp, lq, lse = (torch.full((n,), SENT, dtype=torch.float32, device=DEV) for _ in range(3))
    for t, k, p in ((0.0, 0, 1.0), (-1.0, 0, 1.0), (float("nan"), 0, 1.0), (float("inf"), 0, 1.0), (1.0, 0, 0.0), (1.0, 0, 1.5),
                    (1.0, 0, float("nan")), (1.0, -1, 1.0)):
        with pytest.raises(L.UnimmHipError, match="UNIMM_E_ARG"):
            L.lm_sample(x, n, V, None, None, SR.SEP, t, k, p, KEY, streams, tok, lp, lq, lse)
    L.lm_sample(x, 0, V, None, None, SR.SEP, 1.0, 0, 1.0, KEY, streams, tok, lp, lq, lse)
    torch.cuda.synchronize()
    assert (tok == -7).all() and (lp == SENT).all() and (lq == SENT).all() and (lse == SENT).all()
    got = launch(case["x"], V, V, case["banned"], case["flags"], case["streams"], 1.0, 0, 1.0, rows=0)
    assert got[0].size == 0
