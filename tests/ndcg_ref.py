"""TEST INFRASTRUCTURE: per-slate restatement of NeuralNDCG-transposed in a chosen precision, for the per-element tests of
`unimm_neural_ndcg` (tests/test_gpu_ranking_edges.py; pinned on the CPU by tests/test_ndcg_ref_cpu.py).

It is `unimm_amd.ranking.neuralNDCG_transposed_torch` applied to ONE slate at a time, as the kernel works (one workgroup
per slate, its own stop test), built from the same functions: `ranking.relaxed_sort`, the loop of `ranking.sinkhorn`
(restated here only to count the sweeps and to record the marginals the 1e-8 clamp sees; test_ndcg_ref_cpu.py holds it
bit-equal to `ranking.sinkhorn`), and the discounts / ideal DCG of `ranking.rank_discounts` / `ranking.ideal_dcg` in the
dtype of the inputs instead of fp32.  Returned per slate: the NDCG, whether the slate is alive (has a relevant option), the
autograd gradient of that slate's NDCG with respect to its scores, and the number of sweeps."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from unimm_amd import ranking

Result = namedtuple("Result", "ndcg alive dpred iters clamped unclamped_min")


def rank_discounts(n, k, dtype):
    d = 1.0 / torch.log2(torch.arange(n, dtype=dtype) + 2.0)
    d[k:] = 0.0
    return d


def ideal_dcg(labels, k, pad_label):
    """ranking.ideal_dcg with the discounts in the labels' dtype"""
    y = labels.masked_fill(labels == pad_label, 0.0)
    key = labels.masked_fill(labels == pad_label, -math.inf)
    y = torch.gather(y, 1, key.sort(dim=-1, descending=True)[1])
    n = y.shape[1]
    k = min(k, n)
    d = 1.0 / torch.log2(torch.arange(n, dtype=y.dtype) + 2.0)
    return torch.cumsum(((torch.pow(2.0, y) - 1.0) * d)[:, :k], dim=1)[:, k - 1]


def sinkhorn_counted(mat, pad, tol, max_iter):
    """The loop of ranking.sinkhorn -> (matrix, sweeps, marginals of the unpadded columns / rows that fell below the clamp,
    smallest marginal that did not)."""
    either = pad[:, None, :] | pad[:, :, None]
    both = pad[:, None, :] & pad[:, :, None]
    mat = mat.masked_fill(either, 0.0).masked_fill(both, 1.0)
    valid = ~pad[0]
    clamped, free_min, sweeps = [], math.inf, 0
    for _ in range(max_iter):
        for dim in (1, 2):
            s = mat.sum(dim, keepdim=True)
            sv = s.detach().reshape(-1)[valid]
            low = sv < ranking.EPS
            clamped += sv[low].tolist()
            if bool((~low).any()):
                free_min = min(free_min, float(sv[~low].min()))
            mat = mat / s.clamp(min=ranking.EPS)
        sweeps += 1
        err = torch.maximum((mat.sum(2) - 1.0).abs().max(), (mat.sum(1) - 1.0).abs().max())
        if err < tol:
            break
    return mat.masked_fill(either, 0.0), sweeps, clamped, free_min


def neural_ndcg(pred, truth, pad_label=-1.0, temperature=1.0, powered=True, k=None, max_iter=50, tol=1e-6,
                dtype=torch.float64):
    """pred, truth: [S, n] arrays (any float dtype; converted to `dtype` exactly when it is at least as wide).
    -> Result of numpy arrays: ndcg [S], alive [S], dpred [S, n] (all in `dtype`), iters [S] int, and per slate the list of
    clamped marginals and the smallest unclamped one."""
    pred = torch.as_tensor(np.asarray(pred)).to(dtype)
    truth = torch.as_tensor(np.asarray(truth)).to(dtype)
    S, n = pred.shape
    kk = n if k is None or k <= 0 else k
    out = Result(np.zeros(S, pred.numpy().dtype), np.zeros(S, pred.numpy().dtype), np.zeros((S, n), pred.numpy().dtype),
                 np.zeros(S, np.int64), [[] for _ in range(S)], [math.inf] * S)
    for s in range(S):
        p = pred[s:s + 1].clone().requires_grad_(True)
        y = truth[s:s + 1]
        pad = y == pad_label
        perm = ranking.relaxed_sort(p, temperature, pad)
        perm, sweeps, clamped, free_min = sinkhorn_counted(perm, pad, tol, max_iter)
        out.iters[s] = sweeps
        out.clamped[s] = clamped
        out.unclamped_min[s] = free_min
        exp_disc = torch.einsum("snij,i->snj", perm[None], rank_discounts(n, kk, dtype))
        gains = (torch.pow(2.0, y) - 1.0) if powered else y
        idcg = ideal_dcg(y, kk, pad_label)
        if float(idcg) == 0.0:                       # no relevant option: left out of the mean
            continue
        ndcg = ((gains[None] * exp_disc).sum(2) / (idcg + ranking.EPS)).reshape(())
        out.ndcg[s] = ndcg.detach().numpy()
        out.alive[s] = 1.0
        out.dpred[s] = torch.autograd.grad(ndcg, p)[0][0].numpy()
    return out


def loss_from(res):
    """-(mean NDCG over the alive slates), 0 when none is: what neuralNDCG_transposed returns"""
    alive = res.alive.sum()
    return -(res.ndcg.sum() / alive) if alive > 0 else res.ndcg.dtype.type(0.0)
