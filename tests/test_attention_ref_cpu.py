"""The fp64 attention restatement (oracle/attention_ref.py) against plain dense softmax attention: the packed layout, the
spliced shared segment and dropout each reduce to what they must.  CPU only."""
import math

import numpy as np
import torch

from oracle import attention_ref as AR
from unimm_amd import dropout as DR


def _dense(q, k, v, bits, scale):
    """q [B, H, Tq, D], k / v [B, H, Tk, D], bits bool [B, Tq, Tk] -> out, lse (plain softmax attention, float64)"""
    s = q @ k.transpose(-1, -2) * scale + (~bits).double()[:, None] * -10000.0
    return torch.softmax(s, -1) @ v, torch.logsumexp(s, -1)


def test_packed_equals_padded_dense():
    B, H, Tq, Tk, D = 3, 2, 40, 70, 8
    g = torch.Generator().manual_seed(1)
    ql, kl = [40, 1, 33], [70, 5, 64]
    nw = (Tk + 31) // 32
    bits = torch.rand((B, Tq, nw * 32), generator=g) < 0.6
    bits[:, :, 0] = True
    for b in range(B):
        bits[b, :, kl[b]:] = False                      # cleared past the lengths: the padded run sees the same keys
    words = AR.pack_bits(bits.numpy())                  # [B, Tq, nw]
    q, k, v = (torch.randn((B * T, H * D), generator=g, dtype=torch.float64) for T in (Tq, Tk, Tk))
    dout = torch.randn((B * Tq, H * D), generator=g, dtype=torch.float64)
    for b in range(B):
        dout[b * Tq + ql[b]:(b + 1) * Tq] = 0           # padding queries carry no gradient
    scale = 1 / math.sqrt(D)
    pad = AR.attention(q, k, v, words, B=B, H=H, Tq=Tq, Tk=Tk, D=D, scale=scale, mask_q_stride=nw, mask_b_stride=Tq * nw, dout=dout)
    qh, kh, vh = (x.reshape(B, -1, H, D).transpose(1, 2) for x in (q, k, v))
    ref, ref_lse = _dense(qh, kh, vh, bits[..., :Tk], scale)
    assert torch.allclose(pad["out"], ref.transpose(1, 2).reshape(B * Tq, H * D), atol=1e-12)
    assert torch.allclose(pad["lse"], ref_lse, atol=1e-9)

    qoff = np.concatenate([[0], np.cumsum(ql)[:-1]])
    koff = np.concatenate([[0], np.cumsum(kl)[:-1]]) + 3          # (rows need not start at 0)
    qp = torch.cat([q[b * Tq:b * Tq + ql[b]] for b in range(B)])
    kp = torch.cat([torch.zeros(3, H * D, dtype=torch.float64)] + [k[b * Tk:b * Tk + kl[b]] for b in range(B)])
    vp = torch.cat([torch.zeros(3, H * D, dtype=torch.float64)] + [v[b * Tk:b * Tk + kl[b]] for b in range(B)])
    dp = torch.cat([dout[b * Tq:b * Tq + ql[b]] for b in range(B)])
    words_set = AR.pack_bits(np.where(np.arange(nw * 32) >= np.array(kl)[:, None, None], True, bits.numpy()))
    for w in (words, words_set):                        # bits past k_len must not matter
        pk = AR.attention(qp, kp, vp, w, B=B, H=H, Tq=Tq, Tk=Tk, D=D, scale=scale, mask_q_stride=nw, mask_b_stride=Tq * nw,
                          qvar=(qoff, ql), kvar=(koff, kl), dout=dp)
        for b in range(B):
            r = slice(b * Tq, b * Tq + ql[b])
            assert torch.allclose(pk["out"][qoff[b]:qoff[b] + ql[b]], pad["out"][r], atol=1e-12)
            assert torch.allclose(pk["lse"][b, :, :ql[b]], pad["lse"][b, :, :ql[b]], atol=1e-9)
            assert torch.isnan(pk["lse"][b, :, ql[b]:]).all()
            assert torch.allclose(pk["dq"][qoff[b]:qoff[b] + ql[b]], pad["dq"][r], atol=1e-10)
            rk = slice(b * Tk, b * Tk + kl[b])
            assert torch.allclose(pk["dk"][koff[b]:koff[b] + kl[b]], pad["dk"][rk], atol=1e-10)
            assert torch.allclose(pk["dv"][koff[b]:koff[b] + kl[b]], pad["dv"][rk], atol=1e-10)
        assert float(pk["dk"][:3].abs().max()) == 0.0


def test_spliced_segment_equals_contiguous_keys():
    B, H, D, Tq = 2, 2, 8, 5
    g = torch.Generator().manual_seed(2)
    kl, sl, ins = [6, 3], [4, 7], 1
    Tk = 32
    nw = 1
    bits = torch.rand((B, Tq, 32), generator=g) < 0.7
    bits[:, :, 0] = True
    words = AR.pack_bits(bits.numpy())
    q = torch.randn((B * Tq, H * D), generator=g, dtype=torch.float64)
    k = torch.randn((40, H * D), generator=g, dtype=torch.float64)
    v = torch.randn((40, H * D), generator=g, dtype=torch.float64)
    koff, soff = [0, 6], [20, 30]
    sp = AR.attention(q, k, v, words, B=B, H=H, Tq=Tq, Tk=Tk, D=D, scale=0.3, mask_q_stride=nw, mask_b_stride=Tq * nw,
                      qvar=([0, Tq], [Tq, Tq]), kvar=(koff, kl), kshared=(soff, sl, ins))
    for b in range(B):
        rows = list(range(koff[b], koff[b] + ins)) + list(range(soff[b], soff[b] + sl[b])) + \
            list(range(koff[b] + ins, koff[b] + kl[b]))
        assert list(AR.key_rows(b, koff, kl, soff, sl, ins)) == rows
        n = len(rows)
        qh = q[b * Tq:(b + 1) * Tq].reshape(1, Tq, H, D).transpose(1, 2)
        kh, vh = (x[rows].reshape(1, n, H, D).transpose(1, 2) for x in (k, v))
        ref, ref_lse = _dense(qh, kh, vh, bits[b:b + 1, :, :n], 0.3)
        assert torch.allclose(sp["out"][b * Tq:(b + 1) * Tq], ref[0].transpose(0, 1).reshape(Tq, H * D), atol=1e-12)
        assert torch.allclose(sp["lse"][b], ref_lse[0], atol=1e-9)


def test_dropout_by_hand():
    """One sequence, one head, two queries, three keys: P o keep / (1 - p), keep written out from the device rule."""
    B, H, Tq, Tk, D = 1, 1, 2, 3, 2
    q = torch.tensor([[1.0, 0.0], [0.0, 2.0]], dtype=torch.float64)
    k = torch.tensor([[1.0, 1.0], [0.0, -1.0], [2.0, 0.0]], dtype=torch.float64)
    v = torch.tensor([[1.0, 2.0], [3.0, 5.0], [-1.0, 7.0]], dtype=torch.float64)
    bits = np.array([[[1, 1, 1] + [0] * 29], [[1, 0, 1] + [0] * 29]], dtype=bool).reshape(1, 2, 32)
    p = 0.4
    key = 0x1234567
    drop = DR.drop_arg(p, key)
    res = AR.attention(q, k, v, AR.pack_bits(bits), B=B, H=H, Tq=Tq, Tk=Tk, D=D, scale=1.0, mask_q_stride=1, mask_b_stride=2,
                       drop=drop)
    keep = DR.keep_mask_nd(drop[0], drop[1], (1, 1, 2, 3))[0, 0]
    assert keep.any() and not keep.all()                # both kinds of element occur in this tiny case
    s = np.array([[1.0, 0.0, 2.0], [2.0, -2.0 - 10000.0, 0.0]])
    pr = np.exp(s - s.max(1, keepdims=True))
    pr /= pr.sum(1, keepdims=True)
    pd = pr * keep / (1 - p)
    assert np.allclose(res["probs"][0, 0].numpy(), pd, atol=1e-12)
    assert np.allclose(res["out"].numpy(), pd @ v.numpy(), atol=1e-12)
    assert np.allclose(res["lse"][0, 0].numpy(), np.log(np.exp(s).sum(1)), atol=1e-9)


def test_backward_launch_delta_from_its_out_argument():
    """dq_bwd / dk_bwd / dv_bwd: dS = P o (dP - rowsum(dO o out_arg)) -- the exact gradients when out_arg is the exact output."""
    B, H, Tq, Tk, D = 1, 2, 6, 9, 4
    g = torch.Generator().manual_seed(3)
    q = torch.randn((Tq, H * D), generator=g, dtype=torch.float64)
    k, v = (torch.randn((Tk, H * D), generator=g, dtype=torch.float64) for _ in range(2))
    dout = torch.randn((Tq, H * D), generator=g, dtype=torch.float64)
    words = AR.pack_bits(np.ones((1, 1, 32), dtype=bool))
    kw = dict(B=B, H=H, Tq=Tq, Tk=Tk, D=D, scale=0.5, mask_q_stride=0, mask_b_stride=1, dout=dout)
    exact = AR.attention(q, k, v, words, **kw)
    same = AR.attention(q, k, v, words, out_arg=exact["out"], **kw)
    for n in ("dq", "dk", "dv"):
        assert torch.allclose(same[n + "_bwd"], exact[n], atol=1e-12)
    oa = exact["out"] + 0.01 * torch.randn(exact["out"].shape, generator=g, dtype=torch.float64)
    got = AR.attention(q, k, v, words, out_arg=oa, **kw)
    qh, kh, vh, dh, oh = (x.reshape(-1, H, D).transpose(0, 1) for x in (q, k, v, dout, oa))
    p = torch.softmax(qh @ kh.transpose(1, 2) * 0.5, -1)
    ds = p * (dh @ vh.transpose(1, 2) - (dh * oh).sum(-1, keepdim=True)) * 0.5
    assert torch.allclose(got["dq_bwd"], (ds @ kh).transpose(0, 1).reshape(Tq, H * D), atol=1e-12)
    assert torch.allclose(got["dk_bwd"], (ds.transpose(1, 2) @ qh).transpose(0, 1).reshape(Tk, H * D), atol=1e-12)
    assert torch.allclose(got["dv_bwd"], exact["dv"], atol=1e-12)
    assert not torch.allclose(got["dq_bwd"], exact["dq"], atol=1e-6)
