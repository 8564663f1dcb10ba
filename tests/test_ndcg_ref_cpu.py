"""The per-slate restatement the NeuralNDCG kernel is tested against (tests/ndcg_ref.py), pinned on the CPU: run in fp32 it
reproduces the reference's own values (tests/golden/rankloss.npz) within that file's existing tolerances and equals
`neuralNDCG_transposed_torch`; its counted Sinkhorn loop is bit-equal to `ranking.sinkhorn`; and the two clamp slates of
tests/test_gpu_ranking_edges.py have the properties that file relies on.

Grid searched for a clamped slate with a finite fp32 restatement (clamp_slate: scores gap * permutation(n), pad at 1):
n in {4, 6, 8, 12, 16} x gap in {0.25, 0.5, 1, 1.5, 2, 3} x tau in {0.02, 0.05, 0.1, 0.2}; the conditions (at least one
clamped marginal, every clamped one below 1e-10, every other above 1e-6, finite gradient; fp32 and fp64 alike) hold at
(n >= 6, gap / tau = 25 or 30); CLAMP_FINITE is n = 8, gap = 1.5, tau = 0.05: one clamped marginal of 1.9e-13, the
smallest other 1.9e-5."""
import json
import os

import numpy as np
import pytest
import torch

from tests import ndcg_ref as NR
from tests import test_gpu_ranking_edges as RE
from unimm_amd import ranking

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "rankloss.npz"))
NAMES = [n for n in json.loads(str(G["names"])) if n != "stoch"]


def _kw(name):
    kw = json.loads(str(G[name + "_kw"]))
    kw.pop("seed")
    return kw, dict(temperature=kw.get("temperature", 1.0), powered=kw.get("powered_relevancies", True), k=kw.get("k"))


@pytest.mark.parametrize("name", NAMES)
def test_fp32_restatement_reproduces_the_reference_values(name):
    kw, mine = _kw(name)
    pred, true = G[name + "_pred"], G[name + "_true"]
    res = NR.neural_ndcg(pred, true, dtype=torch.float32, **mine)
    assert res.ndcg.dtype == np.float32 and res.dpred.dtype == np.float32
    np.testing.assert_allclose(NR.loss_from(res), G[name + "_loss"], rtol=2e-5, atol=2e-6)
    grad = -res.dpred / max(res.alive.sum(), 1.0)
    np.testing.assert_allclose(grad, G[name + "_grad"], rtol=2e-4, atol=2e-6)
    # the batched PyTorch formulation: same value within the same tolerances (it stops all slates on one shared test) ...
    p = torch.from_numpy(pred.copy()).requires_grad_(True)
    want = ranking.neuralNDCG_transposed_torch(p, torch.from_numpy(true.copy()), **kw)
    np.testing.assert_allclose(NR.loss_from(res), want.detach().numpy(), rtol=2e-5, atol=2e-6)
    # ... and slate by slate, where both stop on the same test, bit for bit
    for s in range(pred.shape[0]):
        p = torch.from_numpy(pred[s:s + 1].copy()).requires_grad_(True)
        one = ranking.neuralNDCG_transposed_torch(p, torch.from_numpy(true[s:s + 1].copy()), **kw)
        assert float(one.detach()) == -float(res.ndcg[s])
        if res.alive[s]:
            assert np.array_equal(torch.autograd.grad(one, p)[0][0].numpy(), -res.dpred[s])


def test_fp64_restatement_is_close_to_fp32_and_counts_sweeps():
    _, mine = _kw("ragged")
    pred, true = G["ragged_pred"], G["ragged_true"]
    r32 = NR.neural_ndcg(pred, true, dtype=torch.float32, **mine)
    r64 = NR.neural_ndcg(pred, true, dtype=torch.float64, **mine)
    assert r64.ndcg.dtype == np.float64 and np.array_equal(r32.alive, r64.alive)
    assert np.abs(r32.ndcg - r64.ndcg).max() <= 1e-6 and np.abs(r32.dpred - r64.dpred).max() <= 1e-4 * np.abs(r64.dpred).max()
    assert ((1 <= r64.iters) & (r64.iters <= 50)).all()
    fixed = NR.neural_ndcg(pred, true, dtype=torch.float64, max_iter=7, tol=0.0, **mine)
    assert (fixed.iters == 7).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_counted_sinkhorn_is_the_package_loop(dtype):
    g = torch.Generator().manual_seed(5)
    pad = torch.zeros(1, 9, dtype=torch.bool)
    pad[0, 4] = True
    perm = ranking.relaxed_sort(torch.rand(1, 9, generator=g, dtype=dtype), 0.5, pad)
    got, sweeps, clamped, free_min = NR.sinkhorn_counted(perm, pad, 1e-6, 50)
    assert torch.equal(got, ranking.sinkhorn(perm, pad, tol=1e-6, max_iter=50))
    assert torch.equal(got, ranking.sinkhorn(perm, pad, tol=0.0, max_iter=sweeps))
    assert sweeps > 1 and not torch.equal(got, ranking.sinkhorn(perm, pad, tol=0.0, max_iter=sweeps - 1))
    assert clamped == [] and free_min > 1e-3


def test_clamp_slates_have_the_properties_the_gpu_test_relies_on():
    r = RE.refs(RE.CLAMP_N12)
    for res in (r.r32, r.r64):
        assert res.clamped[0] and abs(res.clamped[0][0] - 3.9e-22) < 1e-23           # the first column marginal
    assert np.isnan(r.r32.dpred[0]).any() and np.isfinite(r.r64.dpred[0]).all() and r.r64.alive[0] == 1
    r = RE.refs(RE.CLAMP_FINITE)
    for res in (r.r32, r.r64):
        assert len(res.clamped[0]) >= 1 and max(res.clamped[0]) < 1e-10 and res.unclamped_min[0] > 1e-6
        assert np.isfinite(res.dpred[0]).all() and res.alive[0] == 1
    assert np.isfinite(r.e32).all()


def test_table_has_a_finite_reference_and_a_floor():
    """every gated slate of the GPU table has a finite fp32 restatement; E_FLOOR comes from the tau >= 0.5 cases"""
    for c in RE.CASES + RE.FIXED:
        r = RE.refs(c)
        assert np.isfinite(r.e32).all() and np.isfinite(r.e32n).all(), c.name
        assert r.r64.alive.tolist()[3:5] == [0.0, 0.0] and r.r64.alive[0] == 1 and r.r64.alive[5] == 1, c.name
    assert 1e-7 < RE.e_floor() < 1e-5
