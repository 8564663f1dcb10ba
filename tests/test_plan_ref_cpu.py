"""oracle/plan_ref.py (the integer restatement of unimm_plan_lengths / unimm_plan_build the GPU edge tests compare with)
against the dense formulation written out in tests/test_gpu_kernels.py::test_plan_kernels_match_the_dense_formulation:
the same batches, the same torch expressions, no GPU."""
import numpy as np
import pytest
import torch

from oracle import plan_ref as PR


def dense_batch(B, T, R, two_d, g):
    lens_true = torch.randint(1, T + 1, (B,), generator=g)
    if two_d:
        am = (torch.arange(T)[None, :] < lens_true[:, None]).to(torch.uint8)
    else:
        am = torch.zeros(B, T, T, dtype=torch.uint8)
        for b in range(B):
            n = int(lens_true[b])
            am[b, :n, :n] = (torch.rand(n, n, generator=g) < 0.5).to(torch.uint8)
            am[b, torch.randint(0, n, (1,), generator=g), n - 1] = 1
    cm = torch.zeros(B, R, T, dtype=torch.uint8)
    for b in range(B):
        k = max(1, int(lens_true[b]) - 3)
        cm[b, :, :k] = (torch.rand(R, k, generator=g) < 0.3).to(torch.uint8)
    labels = torch.full((B, T), -1, dtype=torch.int64)
    weights = torch.zeros(B, T, dtype=torch.int64)
    for b in range(B):
        pos = torch.randperm(T, generator=g)[:5]
        labels[b, pos] = torch.randint(0, 1000, (5,), generator=g)
        weights[b, pos[:4]] = torch.tensor([1, -1, 1, -1])
    labels[0, T - 1] = 7
    weights[0, T - 1] = 1
    il = torch.randint(-1, 2, (B, R), generator=g)
    return am, cm, labels, weights, il


@pytest.mark.parametrize("B,T,R,two_d,use_w", [(7, 256, 37, False, True), (5, 64, 37, False, False), (6, 100, 9, True, True),
                                               (3, 256, 256, False, True), (4, 33, 1, False, False)])
def test_plan_ref_equals_the_dense_formulation(B, T, R, two_d, use_w):
    g = torch.Generator().manual_seed(5 + B)
    am, cm, labels, weights, il = dense_batch(B, T, R, two_d, g)
    w = weights if use_w else None
    header = PR.lengths(am.numpy(), cm.numpy(), labels.numpy(), None if w is None else w.numpy(), il.numpy(), B, T,
                        nsp_weight=(5.0, -0.0))
    # the definition on the dense tensors
    valid = am.ne(0) if two_d else (am.ne(0).any(1) | am.ne(0).any(2))
    valid = valid | cm.ne(0).any(1) | labels.ne(-1)
    if use_w:
        valid = valid | weights.ne(0)
    want_len = (valid.int() * torch.arange(1, T + 1)).amax(1).clamp_min(1)
    if not two_d:
        forced = (valid & ~am.ne(0).any(2)).any(1)
        want_len = torch.where(forced, torch.full_like(want_len, T), want_len)
    selm = weights.ne(0) if use_w else labels.ne(-1)
    hh = header.tolist()
    assert hh[:B] == want_len.tolist()
    assert hh[B:2 * B] == selm.sum(1).tolist()
    assert hh[2 * B:2 * B + 2] == [0x40A00000, -0x80000000]          # 5.0 and -0.0 as bit patterns
    assert hh[2 * B + 2:] == il.eq(1).sum(1).tolist()
    Mv, n = sum(hh[:B]), sum(hh[B:2 * B])
    off = torch.cat([torch.zeros(1, dtype=torch.int64), want_len.cumsum(0)[:-1]])
    rows = torch.cat([torch.arange(b * T, b * T + int(l)) for b, l in enumerate(want_len)])
    inv = torch.full((B * T,), -1, dtype=torch.int64)
    inv[rows] = torch.arange(Mv)
    pos = torch.nonzero(selm.reshape(-1))[:, 0]
    for rows_cap, lm_cap in ((None, None), (Mv + 37, n + 5)):
        p = PR.build(header, labels.numpy(), None if w is None else w.numpy(), B, T, rows_cap, lm_cap)
        assert p["off"].tolist() == off.tolist() and p["lens"].tolist() == want_len.tolist()
        assert p["rows"][:Mv].tolist() == rows.tolist() and not p["rows"][Mv:].any()
        assert len(p["rows"]) == (Mv if rows_cap is None else rows_cap)
        assert p["inv"].tolist() == inv.tolist()
        assert p["lm_pos"][:n].tolist() == pos.tolist()
        assert p["lm_idx"][:n].tolist() == inv[pos].tolist()
        assert p["lm_label"][:n].tolist() == labels.reshape(-1)[pos].tolist()
        assert p["lm_weight"][:n].tolist() == (weights.reshape(-1)[pos].tolist() if use_w else [1] * n)
        assert len(p["lm_pos"]) == (n if lm_cap is None else lm_cap)
        assert not p["lm_pos"][n:].any() and not p["lm_idx"][n:].any() and not p["lm_weight"][n:].any()
        assert (p["lm_label"][n:] == -1).all()
        assert p["order"].tolist() == sorted(range(B), key=lambda b: (-int(want_len[b]), b))
        nimg = int(il.eq(1).sum())
        assert p["dims_i"].tolist() == [Mv, n, nimg, 0]
        assert p["dims_f"].dtype == np.float32
        assert p["dims_f"].tolist() == [float(np.float32(1) / np.float32(n)), float(np.float32(1) / np.float32(nimg))]


def test_plan_ref_hostile_sequences_and_omitted_inputs():
    B, T, R = 6, 33, 4
    text = np.zeros((B, T, T), bool)
    co = np.zeros((B, R, T), bool)
    labels = np.full((B, T), -1, np.int64)
    # 0: nothing valid -> 1;  1: valid only through a co-attention bit at 20 (its own row is empty -> full length)
    co[1, 2, 20] = True
    # 2: valid only through a label at T - 1 (own row empty -> T either way);  3: an ordinary prefix of 7
    labels[2, T - 1] = 3
    text[3, :7, :7] = True
    # 4: token 4 attends key 9, whose own row is empty -> full length;  5: key-attended only, own row non-empty
    text[4, 4, 9] = True
    text[5, 2, 2] = True
    h = PR.lengths(text, co, labels, None, None, B, T)
    assert h[:B].tolist() == [1, T, T, 7, T, 3]
    assert h[B:2 * B].tolist() == [0, 0, 1, 0, 0, 0] and not h[2 * B:].any()
    # key-padding and one-row co masks: the bit is the validity, no row can be "empty"
    h = PR.lengths(text[:, 3], co[:, 2], None, None, None, B, T)
    assert h[:B].tolist() == [1, 21, 1, 7, 1, 1]
    # no text mask at all: co-attention and labels still count, and nothing forces the full length
    h = PR.lengths(None, co, labels, None, np.zeros((B, R), np.int64), B, T)
    assert h[:B].tolist() == [1, 21, T, 1, 1, 1]
    p = PR.build(h, None, None, B, T, want_rows=False)
    assert p["rows"] is None and p["inv"] is None and p["lm_pos"] is None
    assert p["dims_i"].tolist() == [21 + T + 4, 0, 0, 0]
    assert p["dims_f"][0] == 1.0 and np.isposinf(p["dims_f"][1])
    with pytest.raises(ValueError):
        PR.build(h, labels, None, B, T, rows_cap=int(h[:B].sum()) - 1)
