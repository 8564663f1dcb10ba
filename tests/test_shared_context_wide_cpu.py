"""Host side of the shared-context pass for answers of up to 30 tokens: `SharedContext` (the permission), `SharedContextPlan` with
the 64-row bound against a brute-force restatement, the launch width chosen per batch, and what stays refused."""
import numpy as np
import pytest
import torch

from tests.test_attention_spliced_cpu import _inputs, _model

T, R = 96, 37


def _plan(groups, c, n, **kw):
    from unimm_amd.scoring import SharedContextPlan
    c, n = np.asarray(c), np.asarray(n)
    return SharedContextPlan(groups, c, n, c + 2 * n, T, R, **kw)


def _brute(gid, c, n, W):
    """rows / prow / lm_idx / lm_pos written out sequence by sequence: the S blocks of the groups in order of first appearance
    (rows 1 .. c - 1 of the group's first member), then per sequence row 0, the answer rows c .. c + n - 1 and the copy rows."""
    B = len(gid)
    seen, rows = [], []
    for b in range(B):
        if gid[b] not in seen:
            seen.append(gid[b])
            rows += [b * T + t for t in range(1, c[b])]
    S = len(rows)
    prow = np.zeros((B, W), dtype=np.int64)
    lm_idx, lm_pos = [], []
    for b in range(B):
        pos = [0] + list(range(c[b], c[b] + 2 * n[b]))
        prow[b, :len(pos)] = pos
        first = len(rows)
        rows += [b * T + t for t in pos]
        lm_idx += [first + 1 + n[b] + k for k in range(n[b])]
        lm_pos += [b * T + c[b] + n[b] + k for k in range(n[b])]
    return S, np.array(rows), prow, np.array(lm_idx), np.array(lm_pos)


def test_plan_with_bound_64_against_brute_force():
    from unimm_amd import SharedContext
    tokens = [0, 13, 14, 15, 16, 30, 14, 0, 30, 15]                  # answers of 0 .. 30 tokens mixed in one call: n = tokens + 1
    gid = [4, 4, 9, 4, 9, 9, 2, 2, 4, 2]
    ctx = {4: 12, 9: 20, 2: 5}
    n = np.array(tokens) + 1
    c = np.array([ctx[g] for g in gid])
    for groups, kw in ((SharedContext(gid, 64), {}), (gid, dict(private_rows=64)), (SharedContext(torch.tensor(gid), 64), {})):
        p = _plan(groups, c, n, **kw)
        S, rows, prow, lm_idx, lm_pos = _brute(gid, c, n, 64)
        assert (p.width, p.private_rows, p.pmax, p.S, p.M) == (64, 64, 63, S, len(rows))
        assert p.prow.shape == (len(gid), 64)
        for name, want in (("rows", rows), ("prow", prow), ("lm_idx", lm_idx), ("lm_pos", lm_pos)):
            assert np.array_equal(getattr(p, name), want), name
        assert p.p_len.tolist() == (1 + 2 * n).tolist() and p.gid.tolist() == [0, 0, 1, 0, 1, 1, 2, 2, 0, 2]


def test_launch_width_follows_the_batch_not_the_permission():
    from unimm_amd import SharedContext
    n = np.array([1, 15, 8])                                         # at most 14 tokens: 31 private rows
    c = np.full(3, 10)
    wide, bare = _plan(SharedContext([0, 0, 1], 64), c, n), _plan([0, 0, 1], c, n)
    assert wide.width == bare.width == 32 and wide.prow.shape == (3, 32)
    for name in ("rows", "prow", "lm_idx", "lm_pos", "p_off", "s_off"):
        assert np.array_equal(getattr(wide, name), getattr(bare, name)), name
    assert _plan(SharedContext([0, 0, 1], 64), c, np.array([1, 16, 8])).width == 64      # one answer of 15 tokens: 33 rows
    assert _plan(SharedContext([0, 0, 1], 32), c, n).width == 32


def test_bounds_and_their_messages():
    from unimm_amd import SharedContext
    c = np.full(2, 10)
    with pytest.raises(ValueError, match=r"65 private rows \(answer of 31 tokens\) exceeds the 64 rows .* 30 tokens"):
        _plan(SharedContext([0, 0], 64), c, np.array([3, 32]))
    assert _plan(SharedContext([0, 0], 64), c, np.array([3, 31])).pmax == 63
    for groups in ([0, 0], torch.tensor([0, 0]), SharedContext([0, 0], 32)):     # the bare list keeps today's refusal, word for word
        with pytest.raises(ValueError, match=r"a candidate with 33 private rows \(answer of 15 tokens\) exceeds one 32-row query tile"):
            _plan(groups, c, np.array([3, 16]))
    with pytest.raises(ValueError, match="private_rows must be 32 or 64"):
        _plan([0, 0], c, np.array([3, 3]), private_rows=48)


def test_shared_context_validation():
    from unimm_amd import SharedContext
    import unimm_amd
    assert "SharedContext" in unimm_amd.__all__ and unimm_amd.scoring.SharedContext is SharedContext
    assert SharedContext([0, 1]).private_rows == 64 and SharedContext([0, 1], 32).private_rows == 32
    assert len(SharedContext([0, 1, 1])) == 3
    inner = SharedContext([0, 1], 32)
    assert SharedContext(inner, 64).groups == [0, 1]                 # wrapping again keeps the ids
    for bad in (0, 16, 33, 63, 65, 128, "64", None, True, 64.5):
        with pytest.raises(ValueError, match="private_rows must be 32 or 64"):
            SharedContext([0, 1], bad)


class _Reached(Exception):
    pass


def test_forward_backward_accepts_the_17_row_answer_when_wrapped():
    """The spec tests/test_attention_spliced_cpu.py shows refused (answers with n = 17 rows: 35 private rows): refused bare, past
    every host check when wrapped (the call is stopped where it would first touch a device)."""
    from unimm_amd import SharedContext
    from unimm_amd.inputs import DialogMaskSpec
    from unimm_amd.scoring import check_shared_training
    args, kw = _inputs()
    kw["attention_mask"] = DialogMaskSpec(np.ones(4), np.full(4, 30), np.full(4, 17))
    grp = torch.tensor([0, 0, 1, 1])
    m = _model()

    def stop(*a, **k):
        raise _Reached()
    m._engine.ensure = stop
    with pytest.raises(ValueError, match="32-row query tile"):
        m.forward_backward(*args, (1.0, 0.0, 0.0), shared_context=grp, **kw)
    with pytest.raises(ValueError, match="32-row query tile"):
        m.forward_backward(*args, (1.0, 0.0, 0.0), shared_context=SharedContext(grp, 32), **kw)
    with pytest.raises(_Reached):
        m.forward_backward(*args, (1.0, 0.0, 0.0), shared_context=SharedContext(grp, 64), **kw)
    chk = lambda g: check_shared_training(m.config, "bf16", (1.0, 0.0, 0.0), kw["attention_mask"], g, 64, 37)
    with pytest.raises(ValueError, match="32-row query tile"):
        chk(grp)
    plan = chk(SharedContext(grp, 64))
    assert (plan.width, plan.pmax, plan.G) == (64, 35, 2)
    with pytest.raises(ValueError, match="one group id"):            # the other refusals look through the wrapper
        chk(SharedContext(grp[:3], 64))


def test_self_critical_step_refuses_more_than_30_tokens_before_any_work():
    from unimm_amd import trainer
    with pytest.raises(ValueError, match="at most 30 tokens"):
        trainer.self_critical_step(None, None, None, {}, {}, 0, None, samples=2, shared_context=True, max_answer_len=31)
