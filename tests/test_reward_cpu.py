"""The CIDEr-D reward without a GPU: tests/reward_ref.py (the float64 restatement of include/unimm_reward.h) against cases worked by
hand, the document-frequency table `unimm_amd.reward` builds against the restated hash and probe, and every refusal of the host
surface (`reward.CiderD`, `reward.NgramTable`, `metrics.cider_d`, `trainer.self_critical_step` with a `DeviceReward`).  No kernel
runs here; tests/test_gpu_reward_edges.py and tests/test_gpu_reward_model.py hold the kernel to the same reference."""
import math

import numpy as np
import pytest
import torch

from tests import reward_ref as R

SEP = 102
A_, B_, C_, D_, E_ = 11, 12, 13, 14, 15


def ans(*toks, width=None):
    """(row, length): tokens, then [SEP], zero padded"""
    row = list(toks) + [SEP]
    return row + [0] * ((width or len(row)) - len(row)), len(row)


def one(h, r, idf=R.unit_idf, sigma=6.0, weights=None):
    refs = r if isinstance(r, list) else [r]
    return R.score_row(h[0], h[1], [x[0] for x in refs], [x[1] for x in refs], weights, idf, sigma)


# ---- the reference against hand-worked cases ---------------------------------------------------------------------------------

@pytest.mark.parametrize("L, want", [(1, 2.5), (2, 5.0), (3, 7.5), (4, 10.0), (7, 10.0)])
def test_a_hypothesis_equal_to_its_only_reference(L, want):
    toks = [A_, B_, C_, D_, E_, A_, C_][:L]
    corpus = [ans(*toks, width=9), ans(77, 78, width=9)]                   # every n-gram of the answer is in 1 of 2 documents
    idf = R.corpus_idf([c[0] for c in corpus], [c[1] for c in corpus])
    assert all(idf(x) == math.log(2.0) for n in range(1, 5) for x in R.windows(toks + [SEP], L + 1, n))
    reward, c = one(ans(*toks), ans(*toks), idf)
    assert reward == pytest.approx(want, rel=1e-12)
    assert c == pytest.approx([1.0 if n <= L else 0.0 for n in range(1, 5)], rel=1e-12)
    assert one(ans(*toks), ans(*toks))[0] == pytest.approx(want, rel=1e-12)          # the no-table form


def test_disjoint_vocabularies_score_zero():
    assert one(ans(A_, B_, C_), ans(D_, E_, 16)) == (0.0, [0.0] * 4)


def test_clipping_closed_form():
    f = math.exp(-4.0 / 72.0)                                               # |L_h - L_r| = 2, sigma = 6
    reward, c = one(ans(A_, A_, A_), ans(A_))                               # v_h = 3, v_r = 1: min(3, 1) * 1 / (3 * 1)
    assert c == pytest.approx([f / 3.0, 0.0, 0.0, 0.0], rel=1e-15) and reward == pytest.approx(10.0 * (f / 3.0) / 4.0, rel=1e-15)
    reward, c = one(ans(A_), ans(A_, A_, A_))                               # v_h = 1, v_r = 3: min(1, 3) * 3 / (1 * 3)
    assert c == pytest.approx([f, 0.0, 0.0, 0.0], rel=1e-15) and reward == pytest.approx(2.5 * f, rel=1e-15)
    # a a b against a b b, idf 1: order 1 (min(2, 1) * 1 + min(1, 2) * 2) / (sqrt 5 * sqrt 5), order 2 (a b) 1 / (sqrt 2 * sqrt 2)
    reward, c = one(ans(A_, A_, B_), ans(A_, B_, B_))
    assert c == pytest.approx([3.0 / 5.0, 1.0 / 2.0, 0.0, 0.0], rel=1e-14)
    assert reward == pytest.approx(10.0 * (0.6 + 0.5) / 4.0, rel=1e-14)


@pytest.mark.parametrize("d", [0, 1, 6])
def test_length_factor(d):
    h, r = ans(A_, *([B_] * d)), ans(A_)
    want = math.exp(-d * d / 72.0) / math.sqrt(1.0 + d * d)                 # order 1: 1 * 1 / (sqrt(1 + d^2) * 1)
    assert one(h, r)[1][0] == pytest.approx(want, rel=1e-15)
    assert one(r, h)[1][0] == pytest.approx(want, rel=1e-15)
    if d == 0:
        assert one(h, r)[1][0] == 1.0


def test_sigma_inf_is_a_factor_of_exactly_one():
    h, r = ans(A_, B_, B_, B_, B_, B_, B_), ans(A_)
    assert one(h, r, sigma=math.inf)[1][0] == 1.0 / math.sqrt(1.0 + 36.0)
    assert one(h, r, sigma=6.0)[1][0] == pytest.approx(math.exp(-0.5) / math.sqrt(37.0), rel=1e-15)


REFS = [ans(A_, B_, C_), ans(A_, B_), ans(C_, C_, D_, E_), ans(B_, C_, D_)]
HYP = ans(A_, B_, C_, D_)


def test_invariance_under_permuting_references():
    w = [0.5, 1.0, 0.0, 2.0]
    base = one(HYP, REFS, weights=w)
    for perm in ([3, 2, 1, 0], [1, 3, 0, 2]):
        got = one(HYP, [REFS[i] for i in perm], weights=[w[i] for i in perm])
        assert got[0] == pytest.approx(base[0], rel=1e-14) and got[1] == pytest.approx(base[1], rel=1e-14)
    assert base[0] > 0


def test_invariance_under_scaling_all_weights():
    w = [0.5, 1.0, 0.25, 2.0]
    base = one(HYP, REFS, weights=w)
    assert one(HYP, REFS, weights=[4.0 * x for x in w]) == base             # a power of two: bit for bit
    assert one(HYP, REFS, weights=[3.0 * x for x in w])[0] == pytest.approx(base[0], rel=1e-14)
    assert one(HYP, REFS, weights=[1.0] * 4) == one(HYP, REFS)              # uniform weights are CIDEr-D's 1 / m


def test_a_zero_weight_reference_equals_its_removal():
    assert one(HYP, REFS, weights=[0.5, 0.0, 0.25, 2.0]) == one(HYP, [REFS[0], REFS[2], REFS[3]], weights=[0.5, 0.25, 2.0])
    assert one(HYP, REFS, weights=[0.0] * 4) == (0.0, [0.0] * 4)            # a weight sum of 0


def test_an_empty_reference_counts_in_the_denominator_and_an_absent_one_does_not():
    full = one(HYP, [REFS[0]])
    empty, absent = ([SEP, 0, 0], 1), ([7, 7, 7], 0)
    assert one(HYP, [REFS[0], empty])[0] == pytest.approx(full[0] / 2.0, rel=1e-15)
    assert one(HYP, [REFS[0], absent]) == full
    assert one(HYP, [absent, absent]) == (0.0, [0.0] * 4)                   # a dialog without a present reference
    assert one(empty, [REFS[0]]) == (0.0, [0.0] * 4) and one(absent, [REFS[0]]) == (0.0, [0.0] * 4)


def test_idf_zero_makes_an_order_vanish_without_a_division_by_zero():
    corpus = [ans(A_, B_, width=5), ans(A_, C_, width=5), ans(D_, A_, width=5)]      # A_ is in every document: idf 0
    idf = R.corpus_idf([c[0] for c in corpus], [c[1] for c in corpus])
    assert idf((A_,)) == 0.0 and idf((B_,)) == math.log(3.0) and idf((A_, B_)) == math.log(3.0) and idf((99,)) == math.log(3.0)
    reward, c = one(ans(A_), ans(A_), idf)                                  # both norms 0: the value stays 0
    assert (reward, c) == (0.0, [0.0] * 4)
    reward, c = one(ans(A_, B_), ans(A_, B_), idf)                          # order 1 lives on B_ alone
    assert c == pytest.approx([1.0, 1.0, 0.0, 0.0], rel=1e-15)


def test_poisoned_tails_are_not_read():
    clean = one(HYP, REFS)
    bad = lambda a: (a[0][:a[1] - 1] + [-7, 65535, A_, B_], a[1])           # noqa: E731   the [SEP] and the tail replaced
    assert one(bad(HYP), [bad(r) for r in REFS]) == clean


# ---- the table builder ---------------------------------------------------------------------------------------------------------

def corpus_arrays(docs, width):
    rows = [ans(*d, width=width) for d in docs]
    return np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.int64)


def test_hash_restatements_agree():
    from unimm_amd import reward, reward_abi
    assert (R.EMPTY, R.HASH_BASIS, R.HASH_PRIME, R.ORDERS) == (reward_abi.EMPTY, reward_abi.HASH_BASIS, reward_abi.HASH_PRIME,
                                                               reward_abi.ORDERS)
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 65536, size=(200, 4))
    keys[::3, 3] = -1
    keys[::5, 2:] = -1
    keys[::7, 1:] = -1
    assert [R.hash_key(tuple(int(v) for v in k)) for k in keys] == reward.ngram_hash(keys).tolist()
    assert R.hash_key((0, -1, -1, -1)) != R.hash_key((0, 0, -1, -1))


def test_df_counts_documents_and_every_ngram_is_where_the_probe_reaches():
    from unimm_amd import reward
    docs = [(A_, A_, A_, B_), (A_, B_), (C_,), (), (A_, A_, A_, A_, A_)]
    tok, ln = corpus_arrays(docs, 8)
    ln[3] = 0                                                               # an absent row is an empty document: it counts in D
    keys, df = reward.corpus_ngrams(tok, ln)
    want, D = R.document_frequencies(tok.tolist(), ln.tolist())
    assert D == 5 and {tuple(k): int(c) for k, c in zip(keys.tolist(), df)} == {R.key_of(x): c for x, c in want.items()}
    assert want[(A_,)] == 3 and want[(A_, A_)] == 2 and want[(A_, A_, A_, A_)] == 1      # documents, not occurrences
    table = reward.NgramTable.from_corpus(tok, ln, device="cpu")
    tk, tv = table.keys.numpy(), table.idf.numpy()
    assert table.num_docs == 5 and table.default_idf == math.log(5.0) and table.cap >= 2 * len(want) and table.cap < 4 * len(want)
    for x, c in want.items():
        slot, found, _ = R.probe(tk, R.key_of(x))
        assert found and tv[slot] == math.log(5.0) - math.log(c)
    assert int((tk[:, 0] != R.EMPTY).sum()) == len(want)
    assert not R.probe(tk, R.key_of((B_, A_)))[1] and R.table_idf(tk, tv, table.default_idf)((B_, A_)) == math.log(5.0)
    idf = R.corpus_idf(tok.tolist(), ln.tolist())
    assert all(R.table_idf(tk, tv, table.default_idf)(x) == idf(x) for x in list(want) + [(B_, A_), (99,)])


def test_a_load_that_forces_probes_to_wrap_past_the_end():
    from unimm_amd import reward
    rng = np.random.default_rng(11)
    keys = np.unique(np.concatenate([rng.integers(0, 30522, size=(16, 1)), np.full((16, 3), -1)], axis=1), axis=0)[:15]
    assert keys.shape == (15, 4)
    values = np.arange(1.0, 16.0)
    tk, tv = reward.build_table(keys, values, max_load=1.0)                 # 15 keys in 16 slots
    assert tk.shape == (16, 4) and int((tk[:, 0] == R.EMPTY).sum()) == 1
    wrapped = 0
    for k, v in zip(keys.tolist(), values):
        slot, found, probes = R.probe(tk, tuple(k))
        assert found and tv[slot] == v
        wrapped += slot < (R.hash_key(tuple(k)) & 15)
    assert wrapped > 0, "no probe wrapped: choose other keys"
    assert not R.probe(tk, (30523, -1, -1, -1))[1]                          # ends at the one empty slot
    tk2, _ = reward.build_table(keys[:8], values[:8], max_load=0.5)
    assert tk2.shape[0] == 16
    with pytest.raises(ValueError, match="cap"):
        reward.build_table(keys, values, cap=8)
    with pytest.raises(ValueError, match="max_load"):
        reward.build_table(keys, values, max_load=0.0)


def test_table_state_dict_round_trip():
    from unimm_amd import reward
    tok, ln = corpus_arrays([(A_, B_, C_), (D_,), (E_,)], 6)
    table = reward.NgramTable.from_corpus(tok, ln, device="cpu")
    assert table.cap == 16 and int((table.keys[:, 0] != R.EMPTY).sum()) == 8            # load 0.5
    other = reward.NgramTable.from_corpus(*corpus_arrays([(A_,)], 3), device="cpu").load_state_dict(table.state_dict())
    assert torch.equal(other.keys, table.keys) and torch.equal(other.idf, table.idf)
    assert (other.default_idf, other.num_docs) == (table.default_idf, 3)
    with pytest.raises(ValueError, match="power of two"):
        reward.NgramTable(torch.zeros((3, 4), dtype=torch.int32), torch.zeros(3, dtype=torch.float64), 0.0, 1)
    with pytest.raises(ValueError, match="lengths"):
        reward.NgramTable.from_corpus(np.zeros((2, 4), np.int64), np.array([5, 1]), device="cpu")


# ---- refusals of the host surface ------------------------------------------------------------------------------------------------

def _good(G=2, N=3, W=6, M=4, Wr=7):
    return dict(tokens=torch.ones((G, N, W), dtype=torch.int64), lengths=torch.full((G, N), 3, dtype=torch.int64),
                reference_tokens=torch.ones((G, M, Wr), dtype=torch.int64), reference_lengths=torch.full((G, M), 4, dtype=torch.int64),
                reference_weights=torch.ones((G, M)))


REFUSALS = [
    ("tokens", lambda k: k.update(tokens=torch.ones((2, 6), dtype=torch.int64))),
    ("lengths", lambda k: k.update(lengths=torch.ones((2, 4), dtype=torch.int64))),
    ("reference_tokens", lambda k: k.update(reference_tokens=torch.ones((3, 4, 7), dtype=torch.int64))),
    ("reference_tokens", lambda k: k.update(reference_tokens=torch.ones((2, 7), dtype=torch.int64))),
    ("reference_lengths", lambda k: k.update(reference_lengths=torch.ones((2, 5), dtype=torch.int64))),
    ("reference_weights", lambda k: k.update(reference_weights=torch.ones((2, 3)))),
    ("lengths", lambda k: k.update(lengths=torch.full((2, 3), 7, dtype=torch.int64))),                     # above its row
    ("reference_lengths", lambda k: k.update(reference_lengths=torch.full((2, 4), 8, dtype=torch.int64))),
    ("lengths", lambda k: k.update(tokens=torch.ones((2, 3, 70), dtype=torch.int64),
                                   lengths=torch.full((2, 3), 66, dtype=torch.int64))),                  # 65 tokens
    ("reference_lengths", lambda k: k.update(reference_tokens=torch.ones((2, 4, 70), dtype=torch.int64),
                                             reference_lengths=torch.full((2, 4), 66, dtype=torch.int64))),
    ("reference_tokens", lambda k: k.update(reference_tokens=torch.ones((2, 129, 7), dtype=torch.int64),
                                            reference_lengths=torch.ones((2, 129), dtype=torch.int64), reference_weights=None)),
    ("reference_weights", lambda k: k.update(reference_weights=torch.tensor([[1.0, -1.0, 1.0, 1.0]] * 2))),
    ("reference_weights", lambda k: k.update(reference_weights=torch.tensor([[1.0, float("nan"), 1.0, 1.0]] * 2))),
    ("reference_weights", lambda k: k.update(reference_weights=torch.tensor([[1.0, float("inf"), 1.0, 1.0]] * 2))),
    ("tokens", lambda k: k.update(tokens=torch.ones((2, 3, 6), dtype=torch.float32))),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_score_refuses_before_anything_is_staged(case, monkeypatch):
    from unimm_amd import reward, reward_abi
    monkeypatch.setattr(reward_abi, "ngram_reward", lambda *a, **k: pytest.fail("a refused call reached the kernel"))
    name, spoil = REFUSALS[case]
    kw = _good()
    spoil(kw)
    with pytest.raises(ValueError, match=name):
        reward.CiderD().score(**kw)


def test_other_refusals(monkeypatch):
    from unimm_amd import metrics, reward, reward_abi
    monkeypatch.setattr(reward_abi, "ngram_reward", lambda *a, **k: pytest.fail("a refused call reached the kernel"))
    for sigma in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            reward.CiderD(sigma=sigma)
    assert reward.CiderD(sigma=math.inf).sigma == math.inf
    with pytest.raises(ValueError, match="table"):
        reward.CiderD(table={"a": 1})
    table = reward.NgramTable.from_corpus(*corpus_arrays([(A_, B_)], 4), device="cpu")     # not on the device the kernel runs on
    with pytest.raises(ValueError, match="table"):
        reward.CiderD(table).score(**_good())
    kw = _good()
    flat = dict(tokens=kw["tokens"].reshape(6, 6), lengths=kw["lengths"].reshape(6), reference_tokens=kw["reference_tokens"],
                reference_lengths=kw["reference_lengths"])
    with pytest.raises(ValueError, match="groups"):
        reward.CiderD().score_rows(groups=torch.tensor([0, 1, 2, 0, 1, 0]), **flat)
    with pytest.raises(ValueError, match="groups"):
        reward.CiderD().score_rows(groups=torch.tensor([0, 1]), **flat)
    with pytest.raises(ValueError, match="lengths"):
        metrics.cider_d(kw["tokens"], kw["lengths"][:, :2], kw["reference_tokens"], kw["reference_lengths"])
    with pytest.raises(ValueError, match="reference_lengths"):
        metrics.cider_d(kw["tokens"][:, 0], kw["lengths"][:, 0], kw["reference_tokens"], kw["reference_lengths"][:, :2])


def test_self_critical_step_with_a_device_reward_and_a_missing_key_raises_before_the_rollout():
    import unimm_amd
    from unimm_amd import reward, trainer

    class Stub(torch.nn.Module):
        def generate_answers(self, *a, **k):
            raise AssertionError("the rollout ran")

    assert unimm_amd.reward is reward and issubclass(reward.CiderD, reward.DeviceReward)
    batch = {"tokens": torch.zeros((2, 8), dtype=torch.int64), "reference_tokens": torch.zeros((2, 3, 5), dtype=torch.int64)}
    with pytest.raises(ValueError, match="reference_lengths"):
        trainer.self_critical_step(Stub(), None, None, batch, {}, 0, reward.CiderD(), samples=2)
    batch = {"tokens": torch.zeros((2, 8), dtype=torch.int64), "reference_lengths": torch.zeros((2, 3), dtype=torch.int64)}
    with pytest.raises(ValueError, match="reference_tokens"):
        trainer.self_critical_step(Stub(), None, None, batch, {}, 0, reward.CiderD(), samples=2, rollout="fused")
