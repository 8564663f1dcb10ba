"""tests/clip_ref.py (the float64 restatement the GPU clipping tests compare with) pinned to torch.nn.utils.clip_grad_norm_ on
CPU float64 tensors, and the public names of the feature: the two entry points and the state struct in the binding's tables,
the two options in FusedAdamW's signature.  No GPU."""
import inspect

import numpy as np
import pytest
import torch

from tests.clip_ref import clip_ref

N = 64 * 40


def table(nc=N // 64, n_groups=8, seed=0):
    return np.random.default_rng(seed).integers(0, n_groups, size=nc).astype(np.uint8)


def torch_clip(g, counted, grad_scale, max_norm):
    """(total norm, coefficient) of clip_grad_norm_ over the counted elements of grad_scale * g, as float64 tensors; the
    coefficient is read off an element of the clipped gradient"""
    x = torch.from_numpy(g[counted].astype(np.float64) * np.float64(np.float32(grad_scale)))
    p = torch.nn.Parameter(torch.zeros_like(x))
    p.grad = x.clone()
    total = torch.nn.utils.clip_grad_norm_([p], max_norm)
    i = int(torch.argmax(x.abs()))
    return float(total), float(p.grad[i] / x[i]) if float(x[i]) != 0.0 else 1.0


def grad(seed=1, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(N) * scale).astype(np.float32)


@pytest.mark.parametrize("grad_scale", [1.0, 0.25, -3.0])
def test_norm_below_max_norm_leaves_the_scale_alone(grad_scale):
    g, eg = grad(scale=1e-3), np.repeat(table(), 64)
    r = clip_ref(g, eg, 8, grad_scale, max_norm=1.0)
    total, coef = torch_clip(g, eg < 8, grad_scale, 1.0)
    assert total < 1.0 and abs(r["norm"] - total) <= 1e-12 * total
    assert r["coef"] == 1.0 and coef == 1.0 and r["nonfinite"] == 0
    assert r["scale"].dtype == np.float32 and r["scale"].tobytes() == np.float32(grad_scale).tobytes()


@pytest.mark.parametrize("grad_scale,max_norm", [(1.0, 1.0), (0.5, 0.3), (3.0, 2.5)])
def test_norm_above_max_norm(grad_scale, max_norm):
    g, eg = grad(), np.repeat(table(), 64)
    r = clip_ref(g, eg, 8, grad_scale, max_norm)
    total, coef = torch_clip(g, eg < 8, grad_scale, max_norm)
    assert total > max_norm
    assert abs(r["norm"] - total) <= 1e-12 * total
    assert abs(r["coef"] - coef) <= 1e-12 * coef and r["coef"] < 1.0
    assert r["coef"] == max_norm / (r["norm"] + 1e-6)
    assert r["scale"] == np.float32(np.float64(np.float32(grad_scale)) * r["coef"])
    assert abs(np.sum(r["group_sumsq"]) - r["sumsq"]) <= 1e-15 * r["sumsq"] and (r["group_sumsq"] > 0).all()


def test_all_zero_gradient():
    r = clip_ref(np.zeros(N, np.float32), np.repeat(table(), 64), 8, 1.0, max_norm=1.0)
    total, coef = torch_clip(np.zeros(N, np.float32), np.ones(N, bool), 1.0, 1.0)
    assert r["norm"] == 0.0 == total and r["coef"] == 1.0 == coef and r["nonfinite"] == 0 and r["scale"] == np.float32(1.0)


def test_elements_whose_fp32_square_overflows():
    g = grad()
    g[[3, 700, N - 1]] = 1e25
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(1e25) * np.float32(1e25))
    eg = np.repeat(table(), 64)
    r = clip_ref(g, eg, 8, 1.0, max_norm=1.0)
    total, coef = torch_clip(g, eg < 8, 1.0, 1.0)
    assert np.isfinite(r["norm"]) and r["nonfinite"] == 0
    assert abs(r["norm"] - total) <= 1e-12 * total and abs(r["coef"] - coef) <= 1e-12 * coef
    assert abs(r["norm"] - np.sqrt(3.0) * float(np.float32(1e25))) <= 1e-12 * r["norm"]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_nonfinite_element_sets_the_flag(bad):
    g = grad()
    g[777] = bad
    r = clip_ref(g, np.repeat(table(), 64), 8, 0.5, max_norm=1.0)
    assert r["nonfinite"] == 1 and r["coef"] == 1.0 and not np.isfinite(r["norm"])
    assert r["scale"].tobytes() == np.float32(0.5).tobytes()


def test_chunks_that_do_not_count_cannot_reach_the_result():
    t = table(n_groups=4)
    t[[2, 9, 17, 30]] = (8, 200, 255, 255)                   # skipped chunks
    t[[5, 11, 23, 39]] = (4, 5, 6, 7)                        # ids in [n_groups, 8): no step, not counted
    eg = np.repeat(t, 64)
    g = grad()
    clean = clip_ref(g, eg, 4, 1.0, max_norm=1.0)
    dirty_g = g.copy()
    dirty_g[eg >= 4] = np.nan
    dirty_g[eg == 255] = np.inf
    dirty = clip_ref(dirty_g, eg, 4, 1.0, max_norm=1.0)
    for k in clean:
        assert np.array_equal(np.asarray(clean[k]), np.asarray(dirty[k])), k
    total, coef = torch_clip(g, eg < 4, 1.0, 1.0)
    assert abs(clean["norm"] - total) <= 1e-12 * total and abs(clean["coef"] - coef) <= 1e-12 * coef
    assert (clean["group_sumsq"][4:] == 0).all() and clean["nonfinite"] == 0
    assert clip_ref(g, eg, 8, 1.0, max_norm=1.0)["sumsq"] > clean["sumsq"]       # with 8 groups, ids 4..7 count


def test_measure_only():
    r = clip_ref(grad(), np.repeat(table(), 64), 8, 2.0, max_norm=np.inf)
    assert r["coef"] == 1.0 and r["scale"] == np.float32(2.0) and r["norm"] > 1.0


def test_the_binding_declares_the_feature():
    import ctypes as C
    from unimm_amd import lib
    from unimm_amd.optim import FusedAdamW
    assert "unimm_grad_norm" in lib.SYMBOLS and "unimm_adamw_step_clipped" in lib.SYMBOLS
    assert "unimm_clip_state" in lib.STRUCTS
    st = lib.STRUCTS["unimm_clip_state"]
    assert [f for f, _ in st._fields_] == ["group_sumsq", "sumsq", "norm", "coef", "scale", "nonfinite", "skipped"]
    assert C.sizeof(st) == 104 and lib.CLIP_STATE_DOUBLES == 13
    assert lib.GRAD_NORM_PASS == 4194304 and lib.GRAD_NORM_WS_DOUBLES == 16384
    sig = inspect.signature(FusedAdamW)
    assert sig.parameters["max_grad_norm"].default is None and sig.parameters["skip_nonfinite"].default is False
