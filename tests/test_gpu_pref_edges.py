"""unimm_seq_pref through the C ABI, per element against the fp64 restatement of its contract (tests/pref_ref.py).

Gate: the kernel forms every sum, the log-sum-exp and c_j in fp64, in the restatement's order, and rounds to fp32 once, so a
result may differ from the restatement's by the rounding (half an fp32 ulp) plus what the device's fp64 exp / log differ from
the host's by -- together at most ONE fp32 ulp of the wanted value, for every element of every output; NaN where the contract
says NaN, exactly 0 where the restatement gives 0.  Nothing is left out.  (The inputs are drawn so that no c_j = beta (w_j - W
P_j) is a cancellation of more than a few digits: a one-ulp difference in an fp64 exp is magnified by W P_j / |w_j - W P_j|,
which would need to reach 1e8 to show in fp32; the saturated case, where the difference is exactly 0, is a case of its own.)

Shapes: 1, 2, 3, 63, 64, 65 and 128 members per group; 0, 1, 2, 63, 64, 65 and 300 rows per sequence; 1 and 5 groups whose members
interleave (sequence k * groups + g is member k of group g); row_seq shuffled; guard elements before and after every output; the
device row count at 0, 1, mid-sequence and n; both length_normalize values; with and without a reference."""
import numpy as np
import pytest
import torch

from tests import pref_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
SENT = np.float32(-12345.678)                    # what an untouched output element holds
ROWS = (1, 2, 63, 64, 65, 300)                   # rows per member, cycled; every group also has one sequence with 0 rows


def L():
    from unimm_amd import lib
    return lib


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def guarded(n):
    return torch.full((n + 2 * GUARD,), float(SENT), dtype=torch.float32, device=DEV)


def inner(t):
    return t[GUARD:t.numel() - GUARD]


def build(members, groups, seed, weights="soft"):
    """`members` sequences with rows + one without per group, interleaved; rows shuffled -> a dict of host arrays"""
    rng = np.random.default_rng(seed)
    B = (members + 1) * groups
    seq_group = (np.arange(B) % groups).astype(np.int32)
    nrows = np.array([0 if j // groups == members else ROWS[(j // groups + j % groups) % len(ROWS)] for j in range(B)])
    row_seq = np.repeat(np.arange(B), nrows).astype(np.int32)
    row_seq = row_seq[rng.permutation(row_seq.shape[0])]
    n = row_seq.shape[0]
    rownll = rng.gamma(2.0, 1.5, n).astype(np.float32)
    ref = (rownll + rng.normal(0, 0.5, n).astype(np.float32)).clip(1e-3).astype(np.float32)
    if weights == "soft":
        w = np.zeros(B, np.float32)
        for g in range(groups):
            idx = np.flatnonzero(seq_group == g)
            e = np.exp(rng.integers(0, 5, idx.shape[0]) * 0.5)
            w[idx] = (e / e.sum()).astype(np.float32)
    else:                                         # one-hot: member 0 of every group
        w = (np.arange(B) < groups).astype(np.float32)
    return dict(rownll=rownll, ref=ref, row_seq=row_seq, seq_group=seq_group, weight=w, B=B, groups=groups, n=n)


def launch(c, beta, lnorm, use_ref, n_dev=None):
    lib = L()
    B, G, n = c["B"], c["groups"], c["n"]
    out = dict(adv=guarded(n), seq_score=guarded(B), seq_prob=guarded(B), group_loss=guarded(G), alive_inv=guarded(1))
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    lib.seq_pref(dev(c["rownll"], torch.float32), dev(c["ref"], torch.float32) if use_ref else None, dev(c["row_seq"], torch.int32), n,
                 dev(c["seq_group"], torch.int32), dev(c["weight"], torch.float32), G, beta, lnorm, inner(out["adv"]),
                 inner(out["seq_score"]), inner(out["seq_prob"]), inner(out["group_loss"]), inner(out["alive_inv"]), n_dev=nd)
    torch.cuda.synchronize()
    host = {}
    for k, t in out.items():
        a = t.cpu().numpy()
        assert (a[:GUARD] == SENT).all() and (a[-GUARD:] == SENT).all(), f"{k}: a guard element was written"
        host[k] = a[GUARD:-GUARD].copy()
    return host


def one_ulp(name, got, want):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (name, "NaN pattern")
    zero = (want == 0.0) & ~nan
    assert (got[zero] == 0.0).all(), (name, "an exact zero is not zero")
    rest = ~nan & ~zero
    if rest.any():
        with np.errstate(over="ignore"):
            w32 = want[rest].astype(np.float32)
        err = np.abs(got[rest].astype(np.float64) - want[rest])
        ulp = np.spacing(np.abs(w32)).astype(np.float64)
        i = int(np.argmax(err / ulp))
        print(f"[pref-edges] {name}: worst {err[i] / ulp[i]:.3g} ulp of {want[rest][i]:.6g} over {int(rest.sum())} elements")
        assert (err <= ulp).all(), (name, float(err[i] / ulp[i]))


def compare(c, got, beta, lnorm, use_ref, n_dev=None):
    rows = c["n"] if n_dev is None else min(c["n"], n_dev)
    want = PR.seq_pref(c["rownll"], c["ref"] if use_ref else None, c["row_seq"], rows, c["seq_group"], c["weight"], c["groups"],
                       beta, lnorm)
    one_ulp("alive_inv", got["alive_inv"], [want["alive_inv"]])
    one_ulp("group_loss", got["group_loss"], want["group_loss"])
    if rows == 0:                                 # nothing else is touched
        for k in ("adv", "seq_score", "seq_prob"):
            assert (got[k] == SENT).all(), k
        return want
    one_ulp("seq_score", got["seq_score"], want["seq_score"])
    one_ulp("seq_prob", got["seq_prob"], want["seq_prob"])
    one_ulp("adv", got["adv"][:rows], want["adv"][:rows])
    assert (got["adv"][rows:] == SENT).all(), "a row past the device count was written"
    return want


@pytest.mark.parametrize("members", [1, 2, 3, 63, 64, 65, 128])
@pytest.mark.parametrize("groups", [1, 5])
def test_every_output_within_one_ulp(members, groups):
    c = build(members, groups, seed=100 * members + groups)
    for lnorm in (False, True):
        for use_ref in (False, True):
            beta = 0.05 if not lnorm else 0.7
            want = compare(c, launch(c, beta, lnorm, use_ref), beta, lnorm, use_ref)
            assert want["alive"].all()
            if members == 1:                      # a one-member group: loss 0, c = 0, P = 1
                assert (want["group_loss"] == 0).all() and (want["adv"] == 0).all()


@pytest.mark.parametrize("n_dev", [0, 1, "mid", "n", "beyond"])
def test_device_row_count(n_dev):
    c = build(3, 2, seed=7)
    nd = {"mid": c["n"] // 2 + 3, "n": c["n"], "beyond": c["n"] + 1000}.get(n_dev, n_dev)
    for lnorm in (False, True):
        compare(c, launch(c, 0.1, lnorm, True, n_dev=nd), 0.1, lnorm, True, n_dev=nd)


def test_no_rows_at_all():
    """n == 0 on the host: UNIMM_OK, alive_inv NaN, group_loss zeroed, nothing else touched"""
    c = build(3, 2, seed=8)
    c = dict(c, n=0)
    got = launch(c, 0.1, False, True)
    assert np.isnan(got["alive_inv"][0]) and (got["group_loss"] == 0).all()
    assert (got["seq_score"] == SENT).all() and (got["seq_prob"] == SENT).all()


def test_dead_groups_by_their_weights():
    """all-zero weights: not alive, loss 0, adv 0 (P is still the softmax); a NaN, an inf and a negative weight: not alive, NaN loss"""
    c = build(3, 5, seed=9)
    w = c["weight"].copy()
    w[c["seq_group"] == 0] = 0.0
    w[np.flatnonzero(c["seq_group"] == 1)[1]] = np.nan
    w[np.flatnonzero(c["seq_group"] == 2)[0]] = -0.25
    w[np.flatnonzero(c["seq_group"] == 3)[2]] = np.inf
    c = dict(c, weight=w)
    got = launch(c, 0.1, True, True)
    want = compare(c, got, 0.1, True, True)
    assert list(want["alive"]) == [False, False, False, False, True] and got["alive_inv"][0] == 1.0
    assert got["group_loss"][0] == 0 and np.isnan(got["group_loss"][1:4]).all() and got["group_loss"][4] > 0
    dead_rows = np.isin(c["seq_group"][c["row_seq"]], (0, 1, 2, 3))
    assert (got["adv"][dead_rows] == 0).all() and (got["adv"][~dead_rows] != 0).any()
    all_dead = dict(c, weight=np.zeros_like(w))
    got = launch(all_dead, 0.1, False, False)
    compare(all_dead, got, 0.1, False, False)
    assert np.isnan(got["alive_inv"][0]) and (got["group_loss"] == 0).all() and (got["adv"] == 0).all()


def test_more_members_than_a_slate_holds():
    """129 members with rows: that group is not alive, NaN loss, its rows 0; its neighbour of 128 is untouched by it"""
    rng = np.random.default_rng(11)
    B = 129 + 128
    seq_group = np.array([0] * 129 + [1] * 128, np.int32)
    perm = rng.permutation(B)
    seq_group = seq_group[perm]
    row_seq = np.repeat(np.arange(B), 2).astype(np.int32)
    row_seq = row_seq[rng.permutation(row_seq.shape[0])]
    n = row_seq.shape[0]
    c = dict(rownll=rng.gamma(2.0, 1.5, n).astype(np.float32), ref=rng.gamma(2.0, 1.5, n).astype(np.float32), row_seq=row_seq,
             seq_group=seq_group, weight=rng.uniform(0.1, 1, B).astype(np.float32), B=B, groups=2, n=n)
    got = launch(c, 0.1, False, True)
    want = compare(c, got, 0.1, False, True)
    assert np.isnan(got["group_loss"][0]) and got["group_loss"][1] > 0 and got["alive_inv"][0] == 1.0
    assert list(want["alive"]) == [False, True]


def test_values_out_of_range_lead_nowhere():
    """row_seq outside [0, B): the row is ignored, adv 0; seq_group outside [0, groups): the sequence is in no group"""
    c = build(3, 2, seed=12)
    rs, sg = c["row_seq"].copy(), c["seq_group"].copy()
    rs[[0, 5, 17]] = (-1, c["B"], 2 ** 31 - 1)
    rs[30] = -2 ** 31
    sg[[2, 3]] = (-1, 2)
    sg[5] = 2 ** 30
    c = dict(c, row_seq=rs, seq_group=sg)
    got = launch(c, 0.1, True, True)
    compare(c, got, 0.1, True, True)
    assert (got["adv"][[0, 5, 17, 30]] == 0).all()
    out = np.isin(c["row_seq"], (2, 3, 5))
    assert (got["adv"][out] == 0).all() and (got["seq_prob"][[2, 3, 5]] == 0).all() and np.isfinite(got["seq_score"][[2, 3, 5]]).all()


def test_saturated_softmax_is_exact_and_finite():
    """z differences of 1e4 and beyond: P exactly 0 / 1, every output finite"""
    c = build(3, 2, seed=13, weights="onehot")
    got = launch(c, 4000.0, False, False)
    want = compare(c, got, 4000.0, False, False)
    z = 4000.0 * want["seq_score"][~np.isnan(want["seq_score"])]
    assert np.ptp(z) >= 1e4
    members = ~np.isnan(want["seq_score"])
    assert set(np.unique(got["seq_prob"][members])) <= {0.0, 1.0} and (got["seq_prob"][members] == 1.0).sum() == 2
    for k in ("adv", "group_loss", "alive_inv", "seq_prob"):
        assert np.isfinite(got[k]).all(), k
    soft = dict(c, weight=build(3, 2, seed=13)["weight"])          # every member weighted: a loss of the order of 1e4, finite
    got = launch(soft, 4000.0, False, False)
    compare(soft, got, 4000.0, False, False)
    assert np.isfinite(got["group_loss"]).all() and got["group_loss"].max() > 1e3


def test_equal_scores_give_the_uniform_distribution():
    c = build(64, 1, seed=14, weights="onehot")
    c = dict(c, rownll=np.full(c["n"], 0.75, np.float32))
    got = launch(c, 0.3, True, False)             # length-normalised: every member scores -0.75
    want = compare(c, got, 0.3, True, False)
    members = ~np.isnan(want["seq_score"])
    assert (got["seq_score"][members] == np.float32(-0.75)).all()
    assert np.unique(got["seq_prob"][members]).size == 1 and abs(float(got["seq_prob"][members][0]) - 1 / 64) <= 2e-9
    assert abs(float(got["group_loss"][0]) - np.log(64.0)) <= 5e-7
    same = dict(c, ref=c["rownll"])               # the reference equals the policy: D = 0 exactly
    got = launch(same, 0.3, False, True)
    compare(same, got, 0.3, False, True)
    assert (got["seq_score"][members] == 0).all()


def test_two_launches_give_the_same_bits():
    c = build(65, 5, seed=15)
    a, b = launch(c, 0.1, True, True), launch(c, 0.1, True, True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_refusals_before_any_launch():
    lib = L()
    c = build(2, 1, seed=16)
    t = lambda a, d: dev(a, d)
    f = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)
    good = dict(rownll=t(c["rownll"], torch.float32), ref_rownll=None, row_seq=t(c["row_seq"], torch.int32), n=c["n"],
                seq_group=t(c["seq_group"], torch.int32), seq_weight=t(c["weight"], torch.float32), groups=1, beta=0.1,
                length_normalize=False, adv=f(c["n"]), seq_score=f(c["B"]), seq_prob=f(c["B"]), group_loss=f(1), alive_inv=f(1))
    lib.seq_pref(**good)
    for bad in (dict(beta=0.0), dict(beta=-1.0), dict(beta=float("inf")), dict(beta=float("nan")), dict(groups=0),
                dict(workspace=torch.zeros(8, dtype=torch.uint8, device=DEV))):
        with pytest.raises(lib.UnimmHipError, match="UNIMM_E_ARG"):
            lib.seq_pref(**dict(good, **bad, group_loss=f(max(bad.get("groups", 1), 1))))
    a = lib.SeqPrefArgs()                          # a NULL required pointer, B < 1
    assert lib.lib().unimm_seq_pref(None, None) == -1
    assert lib.lib().unimm_seq_pref(lib.C.byref(a), None) == -1
    torch.cuda.synchronize()
