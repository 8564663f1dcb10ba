"""CPU checks of oracle/rows_ref.py, the float64 launch semantics the row-edge GPU tests compare against."""
import numpy as np
import torch

from oracle import rows_ref as RR


def test_live_clamps_a_device_count_to_the_capacity():
    assert RR.live(None, 7) == 7
    assert [RR.live(c, 64) for c in (0, 1, 63, 64, 65, 10 ** 6)] == [0, 1, 63, 64, 64, 64]


def test_gather_index_follows_the_row_map():
    assert RR.gather_index(3).tolist() == [0, 1, 2]
    assert RR.gather_index(3, np.array([5, 0, 9, 9])).tolist() == [5, 0, 9]


def test_layernorm_bwd_equals_autograd():
    rng = np.random.default_rng(0)
    M, H = 9, 24
    x = rng.standard_normal((M, H)) * 2 + 1
    gamma = rng.standard_normal(H) * 0.3 + 1
    dy = rng.standard_normal((M, H))
    keep = rng.random((M, H)) > 0.2
    out_keep = rng.random((M, H)) > 0.3
    mean = x.mean(1)
    rstd = 1.0 / np.sqrt(x.var(1) + 1e-12)
    xt = torch.tensor(x, requires_grad=True)
    gt = torch.tensor(gamma, requires_grad=True)
    bt = torch.zeros(H, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.layer_norm(xt, (H,), gt, bt, 1e-12)
    dyt = torch.tensor(np.where(out_keep, dy * 1.25, 0.0))
    y.backward(dyt)
    dx, dxd, dg, db, dbias = RR.layernorm_bwd(dy, x, mean, rstd, gamma, keep, 1.5, out_keep, 1.25)
    assert np.allclose(dx, xt.grad.numpy(), rtol=1e-10, atol=1e-12)
    assert np.allclose(dxd, np.where(keep, xt.grad.numpy() * 1.5, 0.0), rtol=1e-10, atol=1e-12)
    assert np.allclose(dg, gt.grad.numpy(), rtol=1e-10) and np.allclose(db, bt.grad.numpy(), rtol=1e-10)
    assert np.allclose(dbias, dxd.sum(0))


def test_finish_adds_block_sums_and_skips_none():
    blocks, nq, H = 3, 3, 4
    part = np.arange(blocks * nq * H, dtype=np.float32)
    dst0, dst2 = np.ones(H), np.full(H, -2.0)
    (got,) = RR.finish([(part, blocks, H, [dst0, None, dst2])])
    p = part.reshape(blocks, nq, H).astype(np.float64)
    assert got[1] is None
    assert np.array_equal(got[0], 1.0 + p[:, 0].sum(0)) and np.array_equal(got[2], -2.0 + p[:, 2].sum(0))
    # a longer buffer (the capacity of the scratch) is read only up to blocks * nq * H
    (again,) = RR.finish([(np.concatenate([part, np.full(50, np.nan, np.float32)]), blocks, H, [dst0, None, dst2])])
    assert np.array_equal(again[0], got[0])


def test_scatter_add_accumulates_repeated_indices():
    t = RR.scatter_add(np.zeros((3, 2)), [1, 1, 2, 1], np.ones((4, 2)))
    assert t.tolist() == [[0, 0], [3, 3], [1, 1]]


def test_row_and_col_ratio():
    ref = np.array([[1.0, -4.0], [0.0, 0.0], [2.0, 2.0]])
    got = ref + np.array([[0.0, 0.4], [0.0, 0.0], [0.0, 0.2]])
    assert np.allclose(RR.row_ratio(got, ref), [0.1, 0.0, 0.1])
    got[1, 0] = 1e-30
    assert RR.row_ratio(got, ref)[1] == np.inf            # an all-zero reference row must come back exactly zero
    got[2, 1] = np.nan
    assert RR.row_ratio(got, ref)[2] == np.inf
    terms = np.array([[3.0, 1.0], [-3.0, 1.0]])           # column 0 cancels: its sum is gated against the terms' size
    r = RR.col_ratio([0.3, 2.2], terms.sum(0), terms)
    assert np.allclose(r, [0.3 / np.sqrt(18.0), 0.1])
    assert RR.col_ratio([np.nan], [1.0])[0] == np.inf
    assert RR.row_ratio(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)   # a device count of 0 leaves no live rows
