"""What each output of the two-stream encoder may depend on -- TEST INFRASTRUCTURE (CPU, numpy only).

In the reference a masked key carries an additive -10000 (models/vilbert_dialog.py:1415-1431) and exp of that is exactly 0 in
fp32 and in fp64, so the three attention masks of a batch define a hard dependency graph: an output that the graph does not
connect to an input must come back BIT-IDENTICAL when that input changes at unchanged shapes.  This module computes the graph's
closure; tests/test_flow_ref_cpu.py pins it to the float64 oracle in both directions and tests/test_gpu_information_flow.py
holds the engines to it.

Nodes: per sequence b, the T text rows and the R regions.  A text row as an INPUT stands for its token id, position id and type
id; a region for its feature and box rows.  Edges of one block (output <- input):

  text layer        row i   <- row i (residual), and row j where attention_mask[b, i, j] != 0
  image layer       region r <- region r,        and region s where image_attention_mask[b, s] != 0
  connection layer  row i   <- row i,            and region s where image_attention_mask[b, s] != 0   (text queries, image keys)
                    region r <- region r,        and row j where co_attention_mask[b, r, j] != 0       (image queries, text keys)
  a query whose mask row is EMPTY attends every key (all scores carry the same -10000: softmax is shift invariant)
  heads             LM scores of row i <- row i;  image prediction of region r <- region r;  NSP logits <- text row 0 and region 0
                    per-sequence likelihood <- the labelled rows

The blocks are applied in the order of `unimm_amd.params.encoder_schedule(cfg)`; `with_coattention = False` drops the connection
layers.  Every mask is indexed by ONE batch index, so both ends of every edge lie in the same sequence: there is no
cross-sequence edge anywhere.  `Flow.assert_no_cross_sequence` states that on the batch-wide matrix, and `closure` calls it.

For the shared-context schedules nothing of unimm_amd/scoring.py is restated: a group is expanded to the replicated batch's
dense masks (`DialogMaskSpec.dense`) and the closure is computed on that; an input that the members of a group share (the
context, the image) is perturbed in every member."""
from __future__ import annotations

import numpy as np


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def _bmm(a, b):
    """boolean matrix product per sequence"""
    return np.matmul(a.astype(np.uint8), b.astype(np.uint8)) > 0


def dense_masks(attention_mask, image_attention_mask, co_attention_mask, T=None, R=None):
    """The three masks as boolean [B, T, T] (query, key), [B, R] (key) and [B, R, T] (region query, text key); a 2-D text mask
    is a key mask, a 2-D co-attention mask holds for every region."""
    am = _np(attention_mask) != 0
    if am.ndim == 2:
        am = np.broadcast_to(am[:, None, :], (am.shape[0], am.shape[1], am.shape[1]))
    B, T = am.shape[0], am.shape[-1]
    im = np.ones((B, R), dtype=bool) if image_attention_mask is None else _np(image_attention_mask) != 0
    R = im.shape[1]
    cm = np.ones((B, R, T), dtype=bool) if co_attention_mask is None else _np(co_attention_mask) != 0
    if cm.ndim == 2:
        cm = np.broadcast_to(cm[:, None, :], (B, R, T))
    assert am.shape == (B, T, T) and im.shape == (B, R) and cm.shape == (B, R, T), (am.shape, im.shape, cm.shape)
    return am.copy(), im.copy(), cm.copy()


def _attends(mask):
    """[B, Q, K] query-key mask -> the keys each query reads: its set bits, every key when it has none."""
    empty = ~mask.any(-1, keepdims=True)
    return mask | empty


def block_edges(am, im, cm):
    """Edges of one block of each kind, output x input, residual included:
    (text layer [B, T, T], image layer [B, R, R], connection text <- region [B, T, R], connection region <- text [B, R, T])."""
    B, T, R = am.shape[0], am.shape[1], im.shape[1]
    eye_t, eye_v = np.eye(T, dtype=bool)[None], np.eye(R, dtype=bool)[None]
    a_t = _attends(am) | eye_t
    a_v = _attends(np.broadcast_to(im[:, None, :], (B, R, R))) | eye_v
    a_tv = _attends(np.broadcast_to(im[:, None, :], (B, T, R)))
    a_vt = _attends(cm)
    return a_t, a_v, a_tv, a_vt


class Flow:
    """Reachability of a batch, output x input: tt [B, T, T] text row <- text row, tv [B, T, R] text row <- region,
    vt [B, R, T] region <- text row, vv [B, R, R] region <- region."""

    def __init__(self, tt, tv, vt, vv):
        self.tt, self.tv, self.vt, self.vv = tt, tv, vt, vv
        self.B, self.T, self.R = tt.shape[0], tt.shape[1], tv.shape[2]

    # -- forwards: what an input reaches ------------------------------------------------------------
    def from_text(self, b, t):
        """-> dict(text [T], regions [R], nsp): the sequence-output rows (= LM score rows), the image prediction rows and the
        NSP logits of sequence b that text row t may influence.  Nothing of another sequence is reachable."""
        text, regions = self.tt[b, :, t].copy(), self.vt[b, :, t].copy()
        return dict(text=text, regions=regions, nsp=bool(text[0] or regions[0]))

    def from_region(self, b, r):
        text, regions = self.tv[b, :, r].copy(), self.vv[b, :, r].copy()
        return dict(text=text, regions=regions, nsp=bool(text[0] or regions[0]))

    def from_sequence(self, b, text=True, regions=True):
        """what ANY text row (text=True) or region (regions=True) of sequence b reaches"""
        t = np.zeros(self.T, dtype=bool)
        v = np.zeros(self.R, dtype=bool)
        if text:
            t |= self.tt[b].any(1)
            v |= self.vt[b].any(1)
        if regions:
            t |= self.tv[b].any(1)
            v |= self.vv[b].any(1)
        return dict(text=t, regions=v, nsp=bool(t[0] or v[0]))

    def likelihood(self, reach, labelled_b):
        """does the per-sequence likelihood over rows `labelled_b` [T] depend on an input with forward set `reach`"""
        return bool((reach["text"] & _np(labelled_b).astype(bool)).any())

    # -- backwards: where the gradient of a set of outputs may go -----------------------------------
    def to_text_rows(self, b, text_rows=None, regions=None, nsp=False):
        """-> [T] bool: the text INPUT rows of sequence b that the given outputs (text rows [T], regions [R], NSP) read"""
        tr = np.zeros(self.T, dtype=bool) if text_rows is None else _np(text_rows).astype(bool).copy()
        vr = np.zeros(self.R, dtype=bool) if regions is None else _np(regions).astype(bool).copy()
        if nsp:
            tr[0] = vr[0] = True
        return (self.tt[b] & tr[:, None]).any(0) | (self.vt[b] & vr[:, None]).any(0)

    # -- the heart of the matter ---------------------------------------------------------------------
    def batch_matrix(self):
        """The closure over the whole batch, [B * (T + R), B * (T + R)], node (b, text t) = b * (T + R) + t, node (b, region r) =
        b * (T + R) + T + r, assembled edge by edge from the batch indices the masks carry."""
        B, T, R = self.B, self.T, self.R
        N = T + R
        full = np.zeros((B * N, B * N), dtype=bool)
        for name, rows, cols in (("tt", 0, 0), ("tv", 0, T), ("vt", T, 0), ("vv", T, T)):
            b, o, i = np.nonzero(getattr(self, name))
            full[b * N + rows + o, b * N + cols + i] = True        # both ends carry the mask's own batch index b
        return full

    def assert_no_cross_sequence(self):
        full = self.batch_matrix()
        N = self.T + self.R
        seq = np.arange(full.shape[0]) // N
        cross = full & (seq[:, None] != seq[None, :])
        assert not cross.any(), f"{int(cross.sum())} dependencies between different sequences"
        return full


def closure(attention_mask, image_attention_mask, co_attention_mask, cfg, layers=None):
    """The closure of a batch under cfg's encoder schedule -> Flow.
    layers: an explicit block list [("t" | "v" | "c", index), ...] instead of the schedule."""
    from unimm_amd.params import encoder_schedule
    am, im, cm = dense_masks(attention_mask, image_attention_mask, co_attention_mask)
    a_t, a_v, a_tv, a_vt = block_edges(am, im, cm)
    B, T, R = am.shape[0], am.shape[1], im.shape[1]
    tt = np.broadcast_to(np.eye(T, dtype=bool), (B, T, T)).copy()
    vv = np.broadcast_to(np.eye(R, dtype=bool), (B, R, R)).copy()
    tv, vt = np.zeros((B, T, R), dtype=bool), np.zeros((B, R, T), dtype=bool)
    for kind, _ in (encoder_schedule(cfg) if layers is None else layers):
        if kind == "t":
            tt, tv = _bmm(a_t, tt), _bmm(a_t, tv)
        elif kind == "v":
            vt, vv = _bmm(a_v, vt), _bmm(a_v, vv)
        elif kind == "c":
            if not getattr(cfg, "with_coattention", True):
                continue
            tt, tv, vt, vv = tt | _bmm(a_tv, vt), tv | _bmm(a_tv, vv), vt | _bmm(a_vt, tt), vv | _bmm(a_vt, tv)
        else:
            raise ValueError(kind)
    flow = Flow(tt, tv, vt, vv)
    flow.assert_no_cross_sequence()
    return flow


def one_layer(attention_mask, image_attention_mask, co_attention_mask, cfg):
    """The outputs an input reaches through ONE block (the union of the direct edges of the blocks the schedule holds): a subset
    of the closure whose members cannot fail to change when the input does."""
    from unimm_amd.params import encoder_schedule
    am, im, cm = dense_masks(attention_mask, image_attention_mask, co_attention_mask)
    a_t, a_v, a_tv, a_vt = block_edges(am, im, cm)
    kinds = {k for k, _ in encoder_schedule(cfg)}
    if not getattr(cfg, "with_coattention", True):
        kinds.discard("c")
    B, T, R = am.shape[0], am.shape[1], im.shape[1]
    tt = a_t if "t" in kinds else np.broadcast_to(np.eye(T, dtype=bool), (B, T, T)).copy()
    vv = a_v if "v" in kinds else np.broadcast_to(np.eye(R, dtype=bool), (B, R, R)).copy()
    tv = a_tv if "c" in kinds else np.zeros((B, T, R), dtype=bool)
    vt = a_vt if "c" in kinds else np.zeros((B, R, T), dtype=bool)
    flow = Flow(tt.copy(), tv.copy(), vt.copy(), vv.copy())
    flow.assert_no_cross_sequence()
    return flow


def valid_lengths(attention_mask, co_attention_mask=None, labels=None):
    """Rows of each sequence that take part in anything: a row is valid when it attends something, is attended by a row or a
    region, or carries a label (the rule of include/unimm_hip.h's plan) -> [B] lengths of the valid prefixes."""
    am = _np(attention_mask) != 0
    B, T = am.shape[0], am.shape[-1]
    valid = am.any(-1) | am.any(-2) if am.ndim == 3 else am.copy()
    if co_attention_mask is not None:
        cm = _np(co_attention_mask) != 0
        valid = valid | (cm.any(1) if cm.ndim == 3 else cm)
    if labels is not None:
        valid = valid | (_np(labels) != -1)
    return np.array([int(np.nonzero(v)[0].max()) + 1 if v.any() else 1 for v in valid], dtype=np.int64)
