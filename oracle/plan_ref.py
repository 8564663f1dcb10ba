"""Integer restatement of unimm_plan_lengths / unimm_plan_build, written from the text of include/unimm_hip.h (not from
the kernels), for the edge tests (tests/test_gpu_prep_edges.py; pinned to the dense formulation by
tests/test_plan_ref_cpu.py).

Inputs are the DENSE forms of what the kernels read as packed words:
  text    None | bool [B, T, T] (dense: query x key) | bool [B, T] (key-padding: one row per sequence, query stride 0)
  co      None | bool [B, R, T] (region x key)       | bool [B, T] (one row per sequence, query stride 0)
  labels  None | int [B, T] (-1 = no label);  weights  None | int [B, T];  image_label  None | int [B, R]

A token is valid when it attends something, is attended by a token or a region, or carries a label / weight (a key-padding
mask has no queries: its bit is the token's validity).  header[b] is the valid PREFIX length, at least 1; a sequence with a
valid token whose own dense mask row is empty runs at its full length T (such a token attends all T keys uniformly).
Decoded rows: weight != 0 when weights are given, else label != -1; in (sequence, position) order.

Everything is plain Python / numpy integers; dims_f is formed in numpy float32 (one correctly rounded division)."""
from __future__ import annotations

import struct

import numpy as np


def f32_bits(v):
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def lengths(text, co, labels, weights, image_label, B, T, nsp_weight=None):
    """-> header, int32 [3B + 2]: lengths | decoded rows | two NSP weight words (0 when nsp_weight is None) | regions"""
    valid = np.zeros((B, T), bool)
    forced = np.zeros(B, bool)
    empty_row = np.zeros((B, T), bool)
    if text is not None:
        text = np.asarray(text) != 0
        if text.ndim == 2:
            valid |= text
        else:
            valid |= text.any(2) | text.any(1)                    # attends something | is attended by a token
            empty_row = ~text.any(2)
    if co is not None:
        co = np.asarray(co) != 0
        valid |= co if co.ndim == 2 else co.any(1)                # attended by a region
    sel = np.zeros((B, T), bool)
    if labels is not None:
        labels = np.asarray(labels)
        valid |= labels != -1
    if weights is not None:
        weights = np.asarray(weights)
        valid |= weights != 0
    if labels is not None:
        sel = (weights != 0) if weights is not None else (labels != -1)
    forced = (valid & empty_row).any(1)
    header = np.zeros(3 * B + 2, np.int32)
    for b in range(B):
        idx = np.nonzero(valid[b])[0]
        n = int(idx[-1]) + 1 if idx.size else 0
        header[b] = T if forced[b] else max(1, n)
        header[B + b] = int(sel[b].sum())
        header[2 * B + 2 + b] = int((np.asarray(image_label)[b] == 1).sum()) if image_label is not None else 0
    if nsp_weight is not None:
        header[2 * B] = f32_bits(nsp_weight[0])
        header[2 * B + 1] = f32_bits(nsp_weight[1])
    return header


def build(header, labels, weights, B, T, rows_cap=None, lm_cap=None, want_rows=True, want_lm=True):
    """The lists unimm_plan_build writes for capacities that FIT (rows_cap >= sum of lengths, lm_cap >= decoded rows;
    None = exactly the counts).  -> dict(off, lens, rows, inv, lm_pos, lm_idx, lm_label, lm_weight, order, dims_i, dims_f);
    rows / inv are None when want_rows is False, the lm lists when want_lm is False or labels is None."""
    header = [int(v) for v in header]
    lens = header[:B]
    total, nlm, nimg = sum(lens), sum(header[B:2 * B]), sum(header[2 * B + 2:3 * B + 2])
    want_lm = want_lm and labels is not None
    rows_cap = total if rows_cap is None else rows_cap
    lm_cap = nlm if lm_cap is None else lm_cap
    if (want_rows and rows_cap < total) or (want_lm and lm_cap < nlm):
        raise ValueError("plan_ref.build states only plans that fit their capacities")
    off, acc = [], 0
    for n in lens:
        off.append(acc)
        acc += n
    out = dict(off=np.asarray(off, np.int32), lens=np.asarray(lens, np.int32), rows=None, inv=None, lm_pos=None, lm_idx=None,
               lm_label=None, lm_weight=None)
    inv = np.full(B * T, -1, np.int64)
    for b in range(B):
        inv[b * T:b * T + lens[b]] = np.arange(off[b], off[b] + lens[b])
    if want_rows:
        rows = np.zeros(rows_cap, np.int64)                      # tail: index 0
        for b in range(B):
            rows[off[b]:off[b] + lens[b]] = np.arange(b * T, b * T + lens[b])
        out["rows"], out["inv"] = rows, inv
    if want_lm:
        lab = np.asarray(labels).reshape(-1)
        wt = np.asarray(weights).reshape(-1) if weights is not None else None
        pos = np.nonzero(wt != 0 if wt is not None else lab != -1)[0]
        assert len(pos) == nlm, "header and labels / weights disagree"
        lm_pos, lm_idx = np.zeros(lm_cap, np.int32), np.zeros(lm_cap, np.int32)              # tails: index 0,
        lm_label, lm_weight = np.full(lm_cap, -1, np.int32), np.zeros(lm_cap, np.int32)      # label -1, weight 0
        lm_pos[:nlm], lm_idx[:nlm], lm_label[:nlm] = pos, inv[pos], lab[pos]
        lm_weight[:nlm] = wt[pos] if wt is not None else 1
        out.update(lm_pos=lm_pos, lm_idx=lm_idx, lm_label=lm_label, lm_weight=lm_weight)
    out["order"] = np.asarray(sorted(range(B), key=lambda b: (-lens[b], b)), np.int32)       # longest first, ties in batch order
    out["dims_i"] = np.asarray([total, nlm if want_lm else 0, nimg, 0], np.int32)
    with np.errstate(divide="ignore"):
        out["dims_f"] = np.asarray([np.float32(1) / np.float32(max(nlm, 1)), np.float32(1) / np.float32(nimg)], np.float32)
    return out
