"""unimm_ngram_reward (include/unimm_reward.h, libunimm_reward.so) through its C ABI, per element against tests/reward_ref.py, the
float64 restatement of the definition.

Tolerances.  per_order (the c_n, fp64): rtol 1e-12 of the reference, the bound tests/test_gpu_clip_edges.py uses for fp64 sums
against numpy; the chains here have at most 250 terms, all of one sign, and what differs between the two sides is a fused
multiply-add here and there and the last bit of exp and sqrt.  reward (fp32): within one fp32 ulp of float32(reference).

Shapes.  L in {absent, 0, 1, 2, 3, 4, 5, 63, 64} on either side; row strides equal to and above L + 1; M in {1, 2, 3, 100, 128}
with absent references at the start, in the middle and at the end; S in {1, 3, 70} with unsorted groups and a group no row uses;
token ids up to 30521 and 65535; repeated tokens (tf up to L); weights uniform (NULL), one-hot and all zero; the table NULL, over
a vocabulary of 5 ids, at load 0.5 with cap = 16 where a probe wraps past the end, and with n-grams it does not hold.  Every case
fills what lies at and past an answer's effective length, and every absent row, with ids of its own vocabulary: a kernel that
read them would count them.

Properties: two launches give equal bits; a row scored alone equals the same row inside S = 70; S = 0; every refusal returns its
code and leaves the outputs untouched."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import reward_ref as R

pytestmark = pytest.mark.gpu
ARG, SHAPE = -1, -2
SENTINEL = 7.0


def make(seed, hyp_L, ref_L, G, vocab, ldh=None, ldr=None, groups=None, weights=None, copy=0.7, source=None):
    """A case: hyp_L [S] and ref_L [G][M] are effective lengths, -1 = absent.  A hypothesis copies a stretch of a reference of its
    dialog (of reference source[g] where that is given and present) with probability `copy` per token (n-gram overlap), else draws
    from `vocab`.  Everything at and past L is poison."""
    rng = np.random.default_rng(seed)
    vocab = np.asarray(vocab, dtype=np.int64)
    S, M = len(hyp_L), len(ref_L[0])
    ldh = ldh or max(1, max(hyp_L) + 1)
    ldr = ldr or max(1, max(max(r) for r in ref_L) + 1)
    ref = rng.choice(vocab, size=(G, M, ldr))                               # poison everywhere, then nothing to clean
    ref_len = np.array([[L + 1 for L in row] for row in ref_L], dtype=np.int64)
    groups = np.asarray(groups if groups is not None else rng.integers(0, G, S), dtype=np.int64)
    hyp = rng.choice(vocab, size=(S, ldh))
    for s, L in enumerate(hyp_L):
        present = [j for j in range(M) if ref_L[groups[s]][j] > 0]
        if L > 0 and present:
            j = present[int(rng.integers(len(present)))]
            if source is not None and source[groups[s]] in present:
                j = source[groups[s]]
            src = ref[groups[s], j, :ref_L[groups[s]][j]]
            take = rng.random(L) < copy
            hyp[s, :L] = np.where(take, np.resize(src, L), hyp[s, :L])
    hyp_len = np.array([L + 1 for L in hyp_L], dtype=np.int64)
    return dict(hyp=hyp, hyp_len=hyp_len, group=groups, ref=ref, ref_len=ref_len, weight=weights, G=G, M=M, ldh=ldh, ldr=ldr)


def table_of(c, max_load=0.5):
    """the table of the case's references as a corpus (absent rows are empty documents); the hypotheses' own n-grams are absent"""
    from unimm_amd import reward
    G, M, ldr = c["ref"].shape
    return reward.NgramTable.from_corpus(c["ref"].reshape(G * M, ldr), np.maximum(c["ref_len"].reshape(-1), 0), max_load, device="cpu")


def launch(c, table=None, sigma=6.0, per_order=True, rows=None, **override):
    """(return code, reward [S], per_order [S, 4]) of one call through the C ABI; the outputs start as SENTINEL"""
    from unimm_amd import lib as L
    from unimm_amd import reward_abi as A
    dev = torch.device("cuda", 0)
    rows = slice(None) if rows is None else rows
    i32 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev, torch.int32)          # noqa: E731
    t = dict(hyp=i32(c["hyp"][rows]), hyp_len=i32(c["hyp_len"][rows]), group=i32(c["group"][rows]), ref=i32(c["ref"]),
             ref_len=i32(c["ref_len"]))
    t["weight"] = None if c["weight"] is None else torch.from_numpy(np.asarray(c["weight"], dtype=np.float32)).to(dev)
    S = t["hyp_len"].shape[0]
    reward = torch.full((max(S, 1),), SENTINEL, dtype=torch.float32, device=dev)
    orders = torch.full((max(S, 1), 4), SENTINEL, dtype=torch.float64, device=dev)
    a = A.NgramRewardArgs()
    a.hyp, a.hyp_len, a.hyp_group = t["hyp"].data_ptr(), t["hyp_len"].data_ptr(), t["group"].data_ptr()
    a.ref, a.ref_len, a.ref_weight = t["ref"].data_ptr(), t["ref_len"].data_ptr(), L._ptr(t["weight"])
    if table is not None:
        keys, idf = table.keys.to(dev), table.idf.to(dev)
        a.table_keys, a.table_idf, a.cap, a.default_idf = keys.data_ptr(), idf.data_ptr(), keys.shape[0], table.default_idf
    a.reward, a.per_order = reward.data_ptr(), orders.data_ptr() if per_order else None
    a.sigma, a.S, a.ldh, a.G, a.M, a.ldr = sigma, S, c["ldh"], c["G"], c["M"], c["ldr"]
    a.max_hyp_len, a.max_ref_len = min(c["ldh"], 65), min(c["ldr"], 65)
    for k, v in override.items():
        setattr(a, k, v)
    rc = A.lib().unimm_ngram_reward(C.byref(a), L._stream())
    torch.cuda.synchronize()
    return rc, reward.cpu().numpy()[:max(S, 1)], orders.cpu().numpy()


def reference(c, table=None, sigma=6.0):
    idf = R.unit_idf if table is None else R.table_idf(table.keys.numpy(), table.idf.numpy(), table.default_idf)
    return R.score_rows(c["hyp"].tolist(), c["hyp_len"].tolist(), c["group"].tolist(), c["ref"].tolist(), c["ref_len"].tolist(),
                        None if c["weight"] is None else np.asarray(c["weight"], dtype=np.float32).astype(np.float64).tolist(),
                        idf, sigma)


def check(c, table=None, sigma=6.0, what=""):
    rc, reward, orders = launch(c, table, sigma)
    assert rc == 0
    want_r, want_o = reference(c, table, sigma)
    rel = np.abs(orders - want_o) / np.where(want_o != 0, np.abs(want_o), 1.0)
    want32 = want_r.astype(np.float32)
    ulps = np.abs(reward.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
    print(f"\n{what}: S {len(want_r)} reward {want_r.min():.4f} .. {want_r.max():.4f} ({int((want_r > 0).sum())} positive), "
          f"max rel error of c_n {rel.max():.2e}, reward off by at most {ulps.max():.2f} fp32 ulp")
    np.testing.assert_allclose(orders, want_o, rtol=1e-12, atol=0.0)
    assert (ulps <= 1.0).all()
    assert ((want_o == 0) == (orders == 0)).all()
    return reward, orders, want_r


LENGTHS = [-1, 0, 1, 2, 3, 4, 5, 63, 64]
FIVE = [11, 12, 13, 14, 15]


@pytest.mark.parametrize("ldh, ldr", [(65, 65), (80, 71)])
@pytest.mark.parametrize("tabled", [False, True])
def test_every_length_on_either_side(ldh, ldr, tabled):
    """every L against every L, over 5 ids so that tf reaches L and almost every n-gram collides in count"""
    hyp_L = LENGTHS + [64, 5, 3]
    ref_L = [LENGTHS + [4], [64, 63, 5, 0, -1, 2, 2, 1, 64, 3]]
    c = make(1, hyp_L, ref_L, 2, FIVE, ldh, ldr, groups=[0] * 9 + [1, 1, 1])
    c["hyp"][9, :64] = 11                                                   # tf = L = 64 against a reference that repeats too
    c["ref"][1, 0, :64] = np.where(np.arange(64) % 3 == 0, 12, 11)
    table = table_of(c) if tabled else None
    reward, orders, want = check(c, table, what=f"lengths ld {ldh}/{ldr} table {tabled}")
    assert (reward[:2] == 0).all() and (orders[:2] == 0).all() and (want[2:] > 0).all()


@pytest.mark.parametrize("M", [1, 2, 3, 100, 128])
@pytest.mark.parametrize("weights", ["uniform", "onehot", "zero", "random"])
def test_reference_counts_and_weights(M, weights):
    rng = np.random.default_rng(M)
    ref_L = [[int(v) for v in rng.integers(1, 13, M)] for _ in range(2)]
    if M > 1:                                                               # absent at the start, in the middle, at the end
        ref_L[0][0] = ref_L[1][M - 1] = -1
    if M > 2:
        ref_L[0][M // 2] = -1
    if M > 2:
        ref_L[1][1] = 0                                                     # present and empty
    w, source = None, None
    if weights == "onehot":
        w = np.zeros((2, M), dtype=np.float32)
        source = [M - 1, 0]                                                 # present in every M
        w[0, source[0]], w[1, source[1]] = 1.0, 2.5
    elif weights == "zero":
        w = np.zeros((2, M), dtype=np.float32)
    elif weights == "random":
        w = (rng.random((2, M)) * (rng.random((2, M)) < 0.6)).astype(np.float32)
    c = make(100 + M, [7, 3, 12], ref_L, 2, np.arange(1000, 30522), groups=[1, 0, 0], weights=w, ldr=14, source=source)
    reward, orders, want = check(c, table_of(c), what=f"M {M} weights {weights}")
    if weights == "zero":
        assert (reward == 0).all() and (orders == 0).all()
    else:
        assert (want > 0).any()


@pytest.mark.parametrize("S", [1, 3, 70])
@pytest.mark.parametrize("top", [30521, 65535])
def test_row_counts_unsorted_groups_and_wide_ids(S, top):
    rng = np.random.default_rng(S + top)
    groups = rng.choice([3, 0, 1], S)                                       # unsorted; no row uses group 2
    hyp_L = [int(v) for v in rng.integers(-1, 21, S)]
    ref_L = [[int(v) for v in rng.integers(-1, 21, 3)] for _ in range(4)]
    ref_L[3][0] = 20
    vocab = np.concatenate([np.arange(top - 40, top + 1), [0, 1]])
    c = make(7 * S, hyp_L, ref_L, 4, vocab, ldh=24, ldr=21, groups=groups)
    c["hyp"][0, 0] = top
    table = table_of(c) if top == 30521 else None
    reward, _, want = check(c, table, what=f"S {S} ids to {top}")
    assert S == 1 or (want > 0).any()
    again = launch(c, table)
    assert again[1].tobytes() == reward.tobytes()                           # two launches: equal bits
    if S == 70:                                                             # a row alone is the row inside S = 70
        for s in (0, 17, 69):
            rc, r1, o1 = launch(c, table, rows=slice(s, s + 1))
            assert rc == 0 and r1[0].tobytes() == reward[s].tobytes() and o1[0].tobytes() == again[2][s].tobytes()


def wrapping_case():
    """a corpus of 8 n-grams (a b c / a d / an empty and an absent answer: df(a) = 2 of D = 4) whose table at load 0.5 has cap = 16
    and a key that wrapped past the end"""
    from unimm_amd import reward
    for seed in range(400):
        ids = np.random.default_rng(seed).choice(np.arange(200, 30522), 5, replace=False)
        ref_L = [[3, 2, 0, -1]]
        c = make(seed, [3, 2, 4, 1], ref_L, 1, ids, ldr=5)
        c["ref"][0, 0, :3], c["ref"][0, 1, :2] = ids[:3], [ids[0], ids[3]]
        c["hyp"][0, :3] = ids[:3]
        table = table_of(c)
        tk = table.keys.numpy()
        if table.cap == 16 and any(R.probe(tk, tuple(k))[0] < (R.hash_key(tuple(k)) & 15) for k in tk.tolist() if k[0] != R.EMPTY):
            return c, table
    raise AssertionError("no seed gives a wrapped probe")


def test_a_table_whose_probes_wrap_and_ngrams_it_does_not_hold():
    c, table = wrapping_case()
    assert table.cap == 16 and int((table.keys[:, 0] != R.EMPTY).sum()) == 8 and table.num_docs == 4
    reward, orders, want = check(c, table, what="cap 16, load 0.5, a wrapped probe")
    assert want[0] > 0 and orders[0, 2] > 0
    nothing, _, _ = check(c, None, what="the same without a table")
    assert not np.array_equal(nothing, reward)
    for sigma in (math.inf, 0.5):
        check(c, table, sigma=sigma, what=f"sigma {sigma}")


def test_poison_changes_no_bit():
    hyp_L, ref_L = [5, -1, 0, 9], [[4, -1, 0, 7], [-1, -1, 6, 2]]
    c = make(3, hyp_L, ref_L, 2, FIVE, ldh=12, ldr=10, groups=[0, 1, 1, 1])
    table = table_of(c)
    base = launch(c, table)
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    for s, L in enumerate(hyp_L):
        d["hyp"][s, max(L, 0):] = [-5, 65535, 2 ** 31 - 1, 11, 12, 13, 14, 15, 0, 102, 11, 11][max(L, 0):]
    for g in range(2):
        for j, L in enumerate(ref_L[g]):
            d["ref"][g, j, max(L, 0):] = [15, 14, 13, 12, 11, -1, -2, 102, 0, 7][max(L, 0):]
    got = launch(d, table)
    assert got[0] == base[0] == 0 and got[1].tobytes() == base[1].tobytes() and got[2].tobytes() == base[2].tobytes()
    check(d, table, what="poisoned")


def test_no_rows_launch_nothing():
    c = make(5, [3], [[3, 2]], 1, FIVE)
    rc, reward, orders = launch(c, rows=slice(0, 0))
    assert rc == 0 and (reward == SENTINEL).all() and (orders == SENTINEL).all()


def test_per_order_is_optional():
    c = make(5, [3, 4], [[3, 2]], 1, FIVE, groups=[0, 0])
    rc, reward, orders = launch(c, per_order=False)
    assert rc == 0 and (orders == SENTINEL).all() and reward.tobytes() == launch(c)[1].tobytes() and (reward > 0).all()


REFUSED = [
    (ARG, dict(hyp=None)), (ARG, dict(hyp_len=None)), (ARG, dict(hyp_group=None)), (ARG, dict(ref=None)),
    (ARG, dict(ref_len=None)), (ARG, dict(reward=None)), (ARG, dict(table_idf=None)), (ARG, dict(table_keys=None)),
    (ARG, dict(sigma=0.0)), (ARG, dict(sigma=-6.0)), (ARG, dict(sigma=float("nan"))),
    (SHAPE, dict(max_hyp_len=66)), (SHAPE, dict(max_ref_len=66)),          # a length above 64 tokens and the [SEP]
    (SHAPE, dict(max_hyp_len=65, ldh=64)), (SHAPE, dict(max_ref_len=65, ldr=64)),      # a length above the row stride
    (SHAPE, dict(max_hyp_len=-1)), (SHAPE, dict(M=129)), (SHAPE, dict(M=0)), (SHAPE, dict(G=0)), (SHAPE, dict(S=-1)),
    (SHAPE, dict(cap=12)), (SHAPE, dict(cap=0)), (SHAPE, dict(ldh=0)),
]


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_refusals_return_their_code_and_write_nothing(case):
    code, override = REFUSED[case]
    c = make(9, [5, 64, 2], [[3, 64], [2, 2]], 2, FIVE, ldh=70, ldr=70, groups=[0, 1, 0])
    rc, reward, orders = launch(c, table_of(c), **override)
    assert rc == code, (override, rc)
    assert (reward == SENTINEL).all() and (orders == SENTINEL).all()


def test_args_null():
    from unimm_amd import lib as L
    from unimm_amd import reward_abi as A
    assert A.lib().unimm_ngram_reward(None, L._stream()) == ARG
