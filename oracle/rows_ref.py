"""float64 restatement of the launch semantics the row, embedding and weight-gradient kernels share, for the edge tests
(tests/test_gpu_row_edges.py).  Plain math (a LayerNorm, a log-softmax) stays in the tests; what lives here is what a test
would otherwise have to re-derive from the C ABI (include/unimm_hip.h):

  * a device-side count: a launch sized for a CAPACITY reads the real row count from a device word and clamps it with
    min(count, capacity) -- `live`;
  * the packed `rows` map of the unpadded schedule: packed row r reads its ids at index rows[r] -- `gather_index`;
  * the [blocks][nq][H] column-partials layout of unimm_layernorm_bwd_partials and the accumulate (+=) semantics of
    unimm_colpartials_finish_grouped, where dst[q] == None skips quantity q -- `finish`;
  * the per-row and per-column error ratios every gate of the edge tests is stated in -- `row_ratio`, `col_ratio`.

Everything takes and returns numpy arrays (float64 where values are computed)."""
from __future__ import annotations

import numpy as np


def live(count, capacity):
    """Rows a launch with capacity `capacity` and device count `count` (None = no device word) works on."""
    return capacity if count is None else max(0, min(int(count), int(capacity)))


def gather_index(m, rows=None):
    """Index into ids / pos / typ of packed rows 0..m-1: rows[r] when a row map is given, else r."""
    return np.arange(m, dtype=np.int64) if rows is None else np.asarray(rows[:m], dtype=np.int64)


def layernorm_bwd(dy, x, mean, rstd, gamma, keep=None, scale=1.0, out_keep=None, out_scale=1.0):
    """LayerNorm backward of the given rows from the SAVED statistics (what the kernels read), in float64.
    keep / scale: the dropout the forward GEMM epilogue applied on the residual branch (dx_drop = masked dx);
    out_keep / out_scale: dropout the forward applied to y (the upstream gradient is masked first).
    -> dx, dx_drop, dgamma, dbeta, dbias (the last three are column sums over the rows)."""
    dy = np.asarray(dy, np.float64)
    if out_keep is not None:
        dy = np.where(out_keep, dy * out_scale, 0.0)
    xh = (np.asarray(x, np.float64) - np.asarray(mean, np.float64)[:, None]) * np.asarray(rstd, np.float64)[:, None]
    gg = dy * np.asarray(gamma, np.float64)[None, :]
    H = x.shape[1]
    s1 = gg.sum(1, keepdims=True) / H
    s2 = (gg * xh).sum(1, keepdims=True) / H
    dx = np.asarray(rstd, np.float64)[:, None] * (gg - s1 - xh * s2)
    dxd = dx if keep is None else np.where(keep, dx * scale, 0.0)
    return dx, dxd, (dy * xh).sum(0), dy.sum(0), dxd.sum(0)


def partials_sum(partials, blocks, nq, H):
    """Column sums of a [blocks][nq][H] partials buffer -> float64 [nq, H]."""
    p = np.asarray(partials, np.float64).reshape(-1)[: blocks * nq * H].reshape(blocks, nq, H)
    return p.sum(0)


def finish(descs):
    """unimm_colpartials_finish_grouped restated: descs = [(partials, blocks, H, [dst or None, ...])]; returns the new
    value of every destination, in the same nesting (None stays None).  The sums are ADDED to what dst held."""
    out = []
    for part, blocks, H, dsts in descs:
        sums = partials_sum(part, blocks, len(dsts), H)
        out.append([None if d is None else np.asarray(d, np.float64) + sums[q] for q, d in enumerate(dsts)])
    return out


def scatter_add(table, idx, vals):
    """table[idx[r], :] += vals[r, :] for every r (repeated indices accumulate), float64 copy."""
    t = np.array(table, np.float64, copy=True)
    np.add.at(t, np.asarray(idx, np.int64), np.asarray(vals, np.float64))
    return t


def row_ratio(got, ref):
    """Per row: max |got - ref| / max |ref| of that row.  A row whose reference is all zero must be exactly zero
    (its ratio is then 0, else inf).  -> float64 [rows]."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    if got.shape[0] == 0:
        return np.zeros(0)
    got = got.reshape(len(got), -1)
    ref = ref.reshape(len(ref), -1)
    err = np.abs(got - ref).max(1) if got.shape[1] else np.zeros(len(got))
    den = np.abs(ref).max(1) if ref.shape[1] else np.zeros(len(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(got).any(1) if got.shape[1] else False, np.inf, r)


def col_ratio(got, ref, terms=None):
    """Per column of a column sum: |got - ref| / max(|ref|, rss), where rss is the root sum of squares of the column's
    terms (float64 [rows, cols], or None = 0): the expected size of a sum of terms of random sign, so that a column
    whose terms happen to cancel is not held to a relative error of its near-zero sum.  -> float64 [cols]."""
    got = np.asarray(got, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    den = np.abs(ref)
    if terms is not None:
        den = np.maximum(den, np.sqrt((np.asarray(terms, np.float64) ** 2).sum(0)).reshape(-1))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(got), np.inf, r)
