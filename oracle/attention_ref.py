"""fp64 restatement of one attention launch (unimm_attn_fwd / unimm_attn_bwd, include/unimm_hip.h) -- TEST INFRASTRUCTURE.

What one launch computes, for every (sequence b, head h), as the ABI defines it:
  * rows: sequence b owns rows [q_off[b], q_off[b] + q_len[b]) of q / out and key rows of k / v from k_off / k_len (the fixed
    layout is q_off[b] = b Tq, q_len[b] = Tq, likewise for keys);
  * a shared segment (ks_off / ks_len / ks_ins) spliced into the keys: key position j is private row j below ks_ins, then shared
    row j - ks_ins below ks_ins + ks_len[b], else private row j - ks_len[b];
  * keys at positions >= k_len[b] (+ ks_len[b]) do not exist, whatever the mask bits say;
  * the mask: bit j & 31 of word b * mask_b_stride + qi * mask_q_stride + (j >> 5) says key position j may be attended by
    query qi (mask_q_stride = 0: one row per sequence); a cleared bit adds -10000 to the scaled score;
  * dropout: the kept probabilities are scaled by 1 / (1 - p); the keep bit of (b, h, qi, j) is element (b, h, qi, j) of
    unimm_amd.dropout.keep_mask_nd over the PADDED (B, H, Tq, Tk) counters.
out = P V, lse = logsumexp of the masked, scaled scores; dq / dk / dv by autograd on the float64 graph.
"""
from __future__ import annotations

import numpy as np
import torch

from unimm_amd import dropout as DR


def _words(mask) -> np.ndarray:
    """The mask words (int32 / uint32 tensor or array, any shape) as a flat uint32 array."""
    a = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    assert a.dtype.itemsize == 4, a.dtype
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def key_rows(b, k_off, k_len, ks_off=None, ks_len=None, ks_ins=0):
    """Rows of k / v that hold key positions 0 .. n_k - 1 of sequence b (n_k = k_len[b] + ks_len[b])."""
    kl = int(k_len[b])
    if ks_off is None:
        return np.arange(int(k_off[b]), int(k_off[b]) + kl)
    sl, so = int(ks_len[b]), int(ks_off[b])
    j = np.arange(kl + sl)
    return np.where(j < ks_ins, int(k_off[b]) + j, np.where(j < ks_ins + sl, so + j - ks_ins, int(k_off[b]) + j - sl))


def mask_bits(words, b, nq, nk, mask_q_stride, mask_b_stride) -> np.ndarray:
    """bool [nq, nk]: bit (qi, j) of sequence b's mask rows."""
    qi = np.arange(nq)[:, None]
    j = np.arange(nk)[None, :]
    w = words[b * mask_b_stride + qi * mask_q_stride + (j >> 5)]
    return ((w >> (j & 31).astype(np.uint32)) & 1).astype(bool)


def attention(q, k, v, mask, *, B, H, Tq, Tk, D, scale, mask_q_stride, mask_b_stride, qvar=None, kvar=None, kshared=None,
              drop=(0, 0, 1.0), dout=None, out_arg=None):
    """q [rows_q, >= H D], k / v [rows_k, >= H D]: head h = columns h D .. h D + D - 1 (any float dtype, any device); mask: the
    packed words (int32 / uint32, any shape); qvar / kvar = (offsets, lengths) or None (fixed layout); kshared = (ks_off,
    ks_len, ks_ins) or None; drop = (key, thr, scale); dout [rows_q, >= H D] or None.
    Returns float64 CPU tensors: out [rows_q, H D] and lse [B, H, Tq] (rows that no sequence owns: 0 / NaN), probs
    [B, H, Tq, Tk] (the dropped, scaled P at key POSITIONS; 0 where a key does not exist), and with dout also dq [rows_q, H D],
    dk / dv [rows_k, H D] (0 on rows no sequence owns): the exact gradients.
    out_arg [rows_q, >= H D] (or None): the `out` a backward LAUNCH is given.  unimm_attn_bwd forms dS = P o (dP - delta) with
    delta = rowsum(dO o out) of that argument, not of the exact output; dq_bwd / dk_bwd / dv_bwd are the gradients so defined
    (the exact graph plus the term -(delta_arg - delta) . lse, delta_arg - delta held constant: d lse / dS = P).  With a bf16
    `out` they differ from the exact ones by up to a few % of a row whose P is concentrated on one key."""
    HD = H * D
    qd = q[:, :HD].detach().double().cpu().requires_grad_(dout is not None)
    kd = k[:, :HD].detach().double().cpu().requires_grad_(dout is not None)
    vd = v[:, :HD].detach().double().cpu().requires_grad_(dout is not None)
    words = _words(mask)
    if qvar is None:
        q_off, q_len = [b * Tq for b in range(B)], [Tq] * B
    else:
        q_off, q_len = [int(x) for x in qvar[0]], [int(x) for x in qvar[1]]
    if kvar is None:
        k_off, k_len = [b * Tk for b in range(B)], [Tk] * B
    else:
        k_off, k_len = [int(x) for x in kvar[0]], [int(x) for x in kvar[1]]
    ks_off = ks_len = None
    ks_ins = 0
    if kshared is not None:
        ks_off, ks_len, ks_ins = [int(x) for x in kshared[0]], [int(x) for x in kshared[1]], int(kshared[2])
    keep = None
    if drop[1] != 0:
        keep = torch.from_numpy(DR.keep_mask_nd(drop[0], drop[1], (B, H, Tq, Tk)))
    out = torch.zeros((qd.shape[0], HD), dtype=torch.float64)
    lse = torch.full((B, H, Tq), float("nan"), dtype=torch.float64)
    probs = torch.zeros((B, H, Tq, Tk), dtype=torch.float64)
    pieces = []
    for b in range(B):
        nq = q_len[b]
        qr = torch.arange(q_off[b], q_off[b] + nq)
        kr = torch.from_numpy(key_rows(b, k_off, k_len, ks_off, ks_len, ks_ins))
        nk = kr.numel()
        bits = torch.from_numpy(mask_bits(words, b, nq, nk, mask_q_stride, mask_b_stride))
        qh = qd[qr].reshape(nq, H, D).transpose(0, 1)                     # [H, nq, D]
        kh = kd[kr].reshape(nk, H, D).transpose(0, 1)
        vh = vd[kr].reshape(nk, H, D).transpose(0, 1)
        s = qh @ kh.transpose(1, 2) * scale + (~bits).double() * -10000.0
        p = torch.softmax(s, -1)
        lse[b, :, :nq] = torch.logsumexp(s, -1).detach()
        if keep is not None:
            p = p * keep[b, :, :nq, :nk].double() * drop[2]
        probs[b, :, :nq, :nk] = p.detach()
        o = (p @ vh).transpose(0, 1).reshape(nq, HD)
        pieces.append((qr, o, torch.logsumexp(s, -1)))
    for qr, o, _ in pieces:
        out[qr] = o.detach()
    res = dict(out=out, lse=lse, probs=probs)
    if dout is not None:
        dd = dout[:, :HD].detach().double().cpu()
        total = sum((o * dd[qr]).sum() for qr, o, _ in pieces)
        total.backward(retain_graph=out_arg is not None)
        res.update(dq=qd.grad.clone(), dk=kd.grad.clone(), dv=vd.grad.clone())
        if out_arg is not None:
            oa = out_arg[:, :HD].detach().double().cpu()
            for t in (qd, kd, vd):
                t.grad = None
            for qr, o, ls in pieces:
                ddel = ((oa[qr] - o.detach()) * dd[qr]).reshape(-1, H, D).sum(-1).transpose(0, 1)   # [H, nq]
                total = total - (ddel * ls).sum()
            total.backward()
            res.update(dq_bwd=qd.grad, dk_bwd=kd.grad, dv_bwd=vd.grad)
    return res


def pack_bits(bits: np.ndarray) -> np.ndarray:
    """bool [..., nbits] (nbits a multiple of 32) -> uint32 words [..., nbits / 32], bit j & 31 of word j >> 5 = bits[..., j]
    (the layout of unimm_mask_pack)."""
    assert bits.shape[-1] % 32 == 0
    by = np.packbits(bits.astype(np.uint8), axis=-1, bitorder="little")
    return np.ascontiguousarray(by).view(np.uint32)
