"""Generative scoring with the shared dialog context computed once (val_lm.py:52-121).

val_lm.py scores 100 candidate answers per dialog round: the reference builds 100 full sequences
`[CLS] caption [SEP] q1 [SEP] a1 ... q_r [SEP] candidate [SEP] <[MASK] copy of the candidate>` that differ ONLY in the candidate
and runs the whole two-stream encoder on each.  Under the generative mask (utils/data_utils.py:199-210; `oracle/masks.py`
restates it) with L = length incl. candidate + [SEP], n = len(candidate) + 1, c = L - n:

    row 0 (CLS)            attends [0, L + n)
    rows [1, c)  (context) attend  [1, c)            -- never column 0, never the candidate
    rows [c, L)  (answer)  attend  [1, row]
    rows [L, L+n) (copies) attend  [1, row - n) + self
    regions                attend  [1, c)            (co-attention mask)
    every text row         attends all regions

so in EVERY layer the context rows [1, c) and the whole image stream see nothing that depends on the candidate: they are the
same for the 100 sequences of a round.  This module runs them once per group (S rows: c - 1 text rows + the 37 regions) and
only the rows that do depend on the candidate -- row 0, the answer rows and the copy rows: 1 + 2 n of ~140 -- per sequence
(P rows).  All GEMMs / LayerNorms run on one packed row matrix [S_0 | S_1 | ... | P_0 | P_1 | ...]; attention is

    text self-attention     S_g x S_g  (all-ones mask)               one launch over the groups
                            P_b x [CLS_b | S_g(b) | answer_b, copy_b]  one launch over the sequences: the group's K / V rows are
                                                                     SPLICED into each sequence's keys in their original
                                                                     positions (unimm_attn_args.ks_*), masks = the P rows of
                                                                     the sequence's own packed mask
    regions attend text     regions_g x S_g                          (co-attention mask = the context = all of S_g)
    text attends regions    (S_g | P_b) x regions_g(b)               one launch over groups + sequences

TRAINING (`train_shared`, bf16 engine): the same pass with a tape and every dropout site -- N sampled answers of a dialog
(unimm_amd/policy.py) are N sequences of one group, so the context and the image are computed ONCE, forward and backward.  The
blocks below take `st` (train / tape) as `Engine._self_block` / `_conn_block` do and push `(kind, key, fn)` entries that
`Engine._backward_encoder` consumes.  In the backward pass the gradients of the rows a group shares ADD over its sequences:
  text self-attention     the S x S launch's backward (unimm_attn_bwd) writes dQ / dK / dV of the S rows; the spliced launch's
                          backward (unimm_attn_spliced_bwd) then writes the P rows and adds each group's fp32 sums onto the S
                          rows' dK / dV, rounding once
                          (a batch with a sequence of more than 32 private rows, admitted by `SharedContext(ids, 64)`: the
                          same two launches at a width of 64 private rows, unimm_attn_spliced_wide_fwd / _bwd)
  text attends regions    every text block gets its own copy of its group's region K / V rows, unimm_attn_bwd writes one dK / dV
                          copy per block, unimm_segment_rows_sum_bf16 adds a group's copies in list order
  regions attend text     touches S rows only: today's kernel
Only the LM term on the copy rows is trained (any objective of unimm_amd/lm_objective.py); poolers, NSP and image head take no part.

Inference (no tape, no dropout) runs on either engine: the pass is written once against the engine's operand hooks
(unimm_amd/engine.py: `_proj`, `_post_attn`, `_self_block`, `_lm_head`, `_pooled_heads`, and the inference hooks `_ctx_rows` /
`_attn_rows` / `_ctx_operand` / `_embed_image` / `_embed_text`), so on the bf16 engine the rows are bf16 tensors and
on the fp32x3 engine fp32 rows with their split operands (the spliced launch is then unimm_x3_attn_fwd's).  Results equal the
per-sequence path up to the summation order inside the attention kernels (tests/test_gpu_fullsize.py,
tests/test_gpu_x3_scoring.py).  The decoder runs on the copy rows only, as before.  The key/value caches (`cache=`) are
answer generation's and stay with the bf16 engine.
"""
from __future__ import annotations

import numpy as np
import torch

from . import lib as L
from . import lm_objective as LO
from . import params as PM
from .inputs import DialogMaskSpec

BF16, F32 = torch.bfloat16, torch.float32


def _rup(x, m):
    return (x + m - 1) // m * m


class SharedContext:
    """What `shared_context=` takes besides a bare list of group ids: the ids and a PERMISSION -- how many private rows (row 0,
    the answer rows and the copy rows: 1 + 2 (tokens + 1)) a sequence may have.  32 is what a bare list means: answers of up to
    14 tokens, one query tile.  64 admits answers of up to 30 tokens; a call takes the two-tile launches (unimm_attn_spliced_wide_*
    when it trains) only when some sequence of ITS batch has more than 32 private rows, so a call whose answers are all short runs
    the launches of the bare list, bit for bit, dropout included."""

    def __init__(self, groups, private_rows=64):
        if isinstance(private_rows, bool) or private_rows not in (32, 64):
            raise ValueError(f"SharedContext: private_rows must be 32 or 64, got {private_rows!r}")
        if isinstance(groups, SharedContext):
            groups = groups.groups
        self.groups, self.private_rows = groups, int(private_rows)

    def __len__(self):
        return len(self.groups)


def _group_ids(shared_context):
    """-> (group ids int64 [B], bound on the private rows) of a bare id list / tensor or a `SharedContext`"""
    bound = 32
    if isinstance(shared_context, SharedContext):
        shared_context, bound = shared_context.groups, shared_context.private_rows
    if torch.is_tensor(shared_context):
        shared_context = shared_context.cpu().numpy()
    return np.asarray(shared_context, dtype=np.int64).reshape(-1), bound


class SharedContextPlan:
    """Host-side row bookkeeping of one call: which padded rows form the shared (S) and private (P) blocks.
    groups: group ids, or a `SharedContext` (whose bound then replaces `private_rows`); private_rows: the most private rows a
    sequence may have, 32 or 64.  `width` is the launch width of THIS batch: 32 when every sequence fits one query tile, else 64."""

    def __init__(self, groups, c, n, length, T, R, private_rows=32):
        if isinstance(groups, SharedContext):
            groups, private_rows = _group_ids(groups)
        else:
            groups = _group_ids(groups)[0]
        if private_rows not in (32, 64):
            raise ValueError(f"shared_context: private_rows must be 32 or 64, got {private_rows!r}")
        c, n, length = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (c, n, length))
        B = groups.shape[0]
        if not (c.shape[0] == n.shape[0] == length.shape[0] == B):
            raise ValueError("shared_context: one group id / context length / answer length per sequence")
        uniq, first, inv = np.unique(groups, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")                   # groups in order of first appearance
        rank = np.empty_like(order)
        rank[order] = np.arange(order.shape[0])
        self.gid = rank[inv]                                       # [B] group index 0..G-1
        self.rep = first[order]                                    # [G] representative sequence of each group
        G = self.rep.shape[0]
        cg = c[self.rep]
        if (c != cg[self.gid]).any():
            bad = int(np.nonzero(c != cg[self.gid])[0][0])
            raise ValueError(f"shared_context: sequence {bad} has context length {int(c[bad])}, its group's first sequence {int(cg[self.gid[bad]])}")
        if (c < 2).any() or (n < 1).any() or (length != c + 2 * n).any():
            raise ValueError("shared_context: every sequence must be generative-mode [CLS] context answer [SEP] + copy (length = c + 2 n)")
        if (length > T).any():
            raise ValueError("shared_context: truncated copy blocks (length > T) are not supported on this path")
        self.B, self.G, self.T, self.R = B, G, T, R
        self.c, self.n, self.length = c, n, length
        self.s_len = (cg - 1).astype(np.int64)                     # context rows [1, c) of the representative
        self.s_off = np.concatenate([[0], np.cumsum(self.s_len)[:-1]]).astype(np.int64)
        self.S = int(self.s_len.sum())
        self.p_len = (1 + 2 * n).astype(np.int64)                  # row 0 + answer rows + copy rows
        self.p_off = (self.S + np.concatenate([[0], np.cumsum(self.p_len)[:-1]])).astype(np.int64)
        self.P = int(self.p_len.sum())
        self.M = self.S + self.P
        self.pmax = int(self.p_len.max())
        if self.pmax > 32 and private_rows == 32:
            raise ValueError(f"shared_context: a candidate with {self.pmax} private rows (answer of {int(n.max()) - 1} tokens) exceeds one 32-row query tile")
        if self.pmax > 64:
            raise ValueError(f"shared_context: a candidate with {self.pmax} private rows (answer of {int(n.max()) - 1} tokens) exceeds the "
                             "64 rows of two query tiles (answers of at most 30 tokens)")
        self.private_rows = private_rows
        self.width = W = 32 if self.pmax <= 32 else 64             # private rows per sequence in the launches: query tiles x 32
        # packed row -> padded row (b * T + t); vectorised (this runs between the header's arrival and the first launch)
        rows = np.empty(self.M, dtype=np.int64)
        sg = np.repeat(np.arange(G), self.s_len)                   # group of every S row
        rows[:self.S] = self.rep[sg] * T + 1 + (np.arange(self.S) - self.s_off[sg])
        pb = np.repeat(np.arange(B), self.p_len)                   # sequence of every P row
        r = np.arange(self.P) - (self.p_off[pb] - self.S)          # index inside the sequence's private block
        pos = np.where(r == 0, 0, c[pb] + r - 1)                   # row 0, then rows c .. length - 1
        rows[self.S:] = pb * T + pos
        prow = np.zeros((B, W), dtype=np.int64)                    # [B, W] position inside the sequence of private row r (pad: 0)
        prow[pb, r] = pos
        self.rows, self.prow = rows, prow
        # decoded rows: the copy rows = the last n private rows of every sequence, in sequence order
        self.n_lm = int(n.sum())
        lb = np.repeat(np.arange(B), n)
        k = np.arange(self.n_lm) - np.repeat(np.cumsum(n) - n, n)  # index inside the sequence's copy block
        self.lm_idx = self.p_off[lb] + 1 + n[lb] + k               # packed row of each decoded row
        self.lm_pos = lb * T + (length[lb] - n[lb]) + k            # its padded position b * T + t


def check_shared_head_size(cfg, what):
    """The shared pass that TRAINS (a tape, dropout, lse) launches unimm_attn_spliced_fwd / _bwd on the text stream, which take a
    head size of 64 only; inference -- unimm_attn_fwd with a shared segment, unimm_x3_attn_fwd -- takes 64 and 128.  Refused on
    the host, before anything is launched."""
    D = cfg.hidden_size // cfg.num_attention_heads
    if D != 64:
        raise ValueError(f"{what}: text head size {D} (unimm_attn_spliced_fwd / unimm_attn_spliced_bwd take 64)")


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=torch.int32, non_blocking=True)


def _i64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=torch.int64, non_blocking=True)


def forward_shared(eng, inp: dict, groups, want_nsp=True, cache=None):
    """-> dict(rownll [n_lm] fp32, lm_seq [n_lm] int32 (sequence of each decoded row), nsp [B, 2] | None, ok [B] bool, plan).
    `ok[b]` is False where sequence b's context tokens / segments / positions differ from its group's representative (checked on
    the device, no host synchronisation): the caller poisons those scores.
    cache (a dict, or None): also retain what answer generation reads back (unimm_amd/generation.py) -- per text layer key
    't<i>' its fused Q|K|V projection of the packed rows (the S rows are the groups' context K / V), per connection layer key
    'c<i>' the regions' fused projection (K1 / V1), 'vwords' the groups' packed image key masks, and the decoder logits of the
    copy rows in out['logits'].  Nothing computed changes."""
    return eng._on_text_stream(_forward_shared, eng, inp, groups, want_nsp, cache)


def _forward_shared(eng, inp, groups, want_nsp, cache=None, st=None, want_logits=False):
    """st (train / tape, as in `Engine._self_block`): None = inference; with a tape the pass saves for backward, draws every
    dropout mask and returns the LM head's state and the embeddings' backward passes in out['lm'] / out['bwd'].
    want_logits: the decoder logits of the copy rows in out['logits'] WITHOUT the generation caches (the frozen reference of a
    KL-regularised policy step, `Engine._reference_rows`)."""
    cfg = eng.cfg
    st = dict(train=False, tape=None) if st is None else st
    train, tape = st["train"], st["tape"]
    save = tape is not None
    dev = eng.arena.device
    if cache is not None and getattr(eng, "compute_dtype", "bf16") != "bf16":
        raise NotImplementedError("the key/value caches of the shared pass are answer generation's, which runs on the bf16 engine")
    if not cfg.with_coattention:
        raise NotImplementedError("shared-context scoring needs the connection layers (with_coattention)")
    if save:
        check_shared_head_size(cfg, "shared_context training")
    eng.refresh_weights()
    ids = inp["input_ids"]
    B, T = ids.shape
    feat = inp["image_feat"]
    R = feat.shape[1]
    H, Hb = cfg.hidden_size, cfg.bi_hidden_size
    labels = inp.get("masked_lm_labels")
    if labels is None:
        raise ValueError("shared_context scoring needs masked_lm_labels (the copy rows)")
    am = inp.get("attention_mask")
    spec = am if isinstance(am, DialogMaskSpec) else None

    # ---- masks + the per-sequence structure (c, n, length) -------------------------------------------------------------
    eng._dev_masks = []
    if spec is not None:
        if len(spec) != B or int(spec.mode.min()) != 1:
            raise ValueError("shared_context: one generative-mode descriptor per sequence")
        twords, _ = L.mask_synth(*spec.to_device(dev), T)
        nw = twords.shape[-1]
        n_h = spec.answer.astype(np.int64)
        length_h = spec.length.astype(np.int64) + n_h
    else:
        if am is None or am.dim() != 3 or inp.get("co_attention_mask") is None:
            raise ValueError("shared_context scoring needs the dense [B, T, T] generative attention_mask and the co_attention_mask")
        tmask = eng._pack_mask(am, dev, T)
        comask = eng._pack_mask(inp["co_attention_mask"], dev, R)
        twords, nw = tmask[0], tmask[0].shape[-1]
        lab32 = eng._i32(labels.reshape(B, T), dev)
        header = L.plan_lengths(tmask, comask, R, lab32, None, None, B, T)
        hh = header.tolist()                                       # the call's one host synchronisation
        length_h, n_h = np.asarray(hh[:B]), np.asarray(hh[B:2 * B])
    eng._dev_masks = []
    c_h = np.asarray(length_h) - 2 * np.asarray(n_h)
    plan = SharedContextPlan(groups, c_h, n_h, length_h, T, R)
    G, M, S, W = plan.G, plan.M, plan.S, plan.width
    eng._step_rows = M
    eng.last_plan = None

    rows = _i64(plan.rows, dev)
    s_off, s_len = _i32(plan.s_off, dev), _i32(plan.s_len, dev)
    p_off, p_len = _i32(plan.p_off, dev), _i32(plan.p_len, dev)
    gid = _i64(plan.gid, dev)
    rep = _i64(plan.rep, dev)
    ks_off, ks_len = s_off[gid], s_len[gid]                        # [B]: the group's rows, per sequence
    # item order of the candidates' launches: most keys first (unimm_attn_args.order: the tail of a launch is its shortest items)
    p_ord = _i32(np.argsort(-(plan.s_len[plan.gid] + plan.p_len), kind="stable"), dev)
    # P-row masks: rows {0, c .. length) of each sequence's packed mask, key positions unchanged
    prow = _i64(plan.prow, dev)                                    # [B, W]
    pwords = twords.view(B, T, nw)[torch.arange(B, device=dev)[:, None], prow].contiguous()        # [B, W, nw]
    ones_t = torch.full((G, nw), -1, dtype=torch.int32, device=dev)                                # all-ones key masks (lengths bound them)

    # ---- is the context really shared?  (device-side check, folded into `ok`) -----------------------------------------
    tt, pp = inp.get("token_type_ids"), inp.get("position_ids")
    ids_d = ids.to(dev, non_blocking=True)
    col = torch.arange(T, device=dev)[None, :]
    c_d = _i64(plan.c, dev)[:, None]
    ctx_cols = (col >= 1) & (col < c_d)
    same = ((ids_d == ids_d[rep[gid]]) | ~ctx_cols).all(1)
    for t in (tt, pp):
        if t is not None:
            t_d = t.to(dev, non_blocking=True)
            same &= ((t_d == t_d[rep[gid]]) | ~ctx_cols).all(1)
    lab_d = labels.to(dev, non_blocking=True)
    len_d = _i64(plan.length, dev)[:, None]
    n_d = _i64(plan.n, dev)[:, None]
    copy_cols = (col >= len_d - n_d) & (col < len_d)
    same &= ((lab_d != -1) == copy_cols).all(1)                    # the labelled rows are exactly the copy rows
    if spec is None:
        # The S rows run with an all-ones mask bounded by their length and the regions attend them the same way: that IS the
        # generative mask's context block (utils/data_utils.py:199-210: rows and columns [1, c) fully connected, nothing else
        # visible to a context row; co-attention keys [1, c)) -- checked here instead of assumed: a dense mask that deviates in
        # the context block, or a non-generative row, gives NaN instead of a silently different score.
        colw = torch.arange(nw * 32, device=dev).view(1, nw, 32)
        bits = ((colw >= 1) & (colw < c_d[:, :, None])).to(torch.int64)                        # [B, nw, 32]
        expw = (bits << torch.arange(32, device=dev)).sum(-1)
        expw = torch.where(expw >= 2 ** 31, expw - 2 ** 32, expw).to(torch.int32)                 # the packed words of columns [1, c)
        same &= ((twords.view(B, T, nw) == expw[:, None, :]).all(-1) | ~ctx_cols).all(1)
        same &= (comask[0].view(B, -1, nw) == expw[:, None, :]).all(-1).all(1)
    img_idx = inp.get("image_index")
    if img_idx is not None:
        img_idx = img_idx.to(dev, dtype=torch.int64, non_blocking=True).reshape(-1)
        same &= img_idx == img_idx[rep[gid]]
        img_rows = img_idx[rep]                                    # [G] entry of the per-image tensors
    else:
        if feat.shape[0] != B:
            raise ValueError(f"image_feat has {feat.shape[0]} rows for {B} sequences and no image_index was given")
        img_rows = rep

    NO = L.NO_DROP
    # ---- image embedding, one per group (image stream) -----------------------------------------------------------------
    F = cfg.v_feature_size
    im = inp.get("image_attention_mask")
    feat_d = feat.to(dev, non_blocking=True)
    loc_d = inp["image_loc"].to(dev, non_blocking=True)
    if img_idx is None:                                            # per-sequence copies (val_lm.py:78-91 expands them): every member
        fv, lv = feat_d.reshape(B, -1), loc_d.reshape(B, -1)       # must carry its group's image -- compared in full on the device
        same &= (fv == fv[rep[gid]]).all(1) & (lv == lv[rep[gid]]).all(1)
    eng._to_img()
    with eng._img():
        featd = feat_d.index_select(0, img_rows).to(F32).contiguous().view(G * R, F)
        locd = loc_d.index_select(0, img_rows).to(F32).contiguous().view(G * R, 5)
        xv32, xv, bwd_embv = eng._embed_image(featd, locd, G * R, eng._drop("emb_v", cfg.hidden_dropout_prob, train), save)
    if im is None:
        im = torch.ones((B, R), dtype=torch.uint8, device=dev)
    imd = im.to(dev, non_blocking=True)
    if imd.dim() == 2:
        same &= (imd == imd[rep[gid]]).all(1)                      # ... and its group's image key mask
    eng._dev_masks = []
    vmask = eng._pack_mask(imd.index_select(0, rep), dev, R)       # [G] image key masks
    eng._dev_masks = []
    if vmask[1] != 0:
        raise ValueError("shared_context: image_attention_mask must be a [B, R] key mask")
    nwv = vmask[0].shape[-1]

    # ---- text embeddings on the packed rows -----------------------------------------------------------------------------
    ids32 = eng._i32(ids.reshape(-1), dev)
    typ32 = eng._i32(tt.reshape(-1), dev) if tt is not None else torch.zeros(B * T, dtype=torch.int32, device=dev)
    pos32 = eng._i32(pp.reshape(-1), dev) if pp is not None else torch.arange(T, dtype=torch.int32, device=dev).repeat(B)
    d_embt = eng._drop("emb_t", cfg.hidden_dropout_prob, train)
    xt32, xt, _ = eng._embed_text(ids32, pos32, typ32, M, rows, d_embt, False, None)
    # (the step's embedding backward scatters with fp32 atomics; this one adds in a fixed order: the step repeats bit for bit)
    bwd_embt = eng._embed_text_bwd_ordered(ids32, pos32, typ32, M, rows, d_embt) if save else None

    heads, D = cfg.num_attention_heads, H // cfg.num_attention_heads
    nh, Db = cfg.bi_num_attention_heads, Hb // cfg.bi_num_attention_heads
    # items of the text-attends-regions launch: the groups' S blocks, then the sequences' P blocks
    it_off, it_len = torch.cat([s_off, p_off]), torch.cat([s_len, p_len])
    it_img = torch.cat([torch.arange(G, device=dev), gid]).to(torch.int32)
    it_koff = it_img * R
    it_klen = torch.full_like(it_koff, R)
    it_vwords = vmask[0].view(G, nwv)[it_img.long()].contiguous()                                  # [G + B, nwv]

    if save:
        # the groups of the spliced backward launch, and of the region sums: item g (the group's S block) then G + b of its members
        g_first, g_seq = L.group_lists(plan.gid, G)
        groups_dev = (_i32(g_first, dev), _i32(g_seq, dev))
        it_first = _i32(g_first + np.arange(G + 1), dev)
        it_seq = _i32(np.concatenate([np.concatenate([[g], G + g_seq[g_first[g]:g_first[g + 1]]]) for g in range(G)]), dev)
        rep_rows = (it_img.long()[:, None] * R + torch.arange(R, device=dev)[None, :]).reshape(-1).to(torch.int32)
        rep_koff = torch.arange(G + B, dtype=torch.int32, device=dev) * R

    def train_kw(drop, lse):
        """what a training pass adds to an `_attn_rows` launch (inference passes nothing: both engines take the call)"""
        return dict(drop=drop, lse=lse) if save else {}

    # (x32, x) below: an fp32 residual stream and its copy as the engine's GEMM operand, as in `Engine._self_block`
    def text_block(key, i, x32, x):
        """BertLayer (models/vilbert_dialog.py:385-483) on the packed rows."""
        pn = f"bert.encoder.layer.{i}."
        qkv_l, so, ff1, ff2 = (eng.lin[key + s] for s in (".qkv", ".so", ".ff1", ".ff2"))
        qkv = eng._proj(x, qkv_l)
        if cache is not None:
            cache[key] = qkv
        q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
        ctx = eng._ctx_rows(M, H, dev)
        # (two launches, two dropout sites: their counters both start at item 0)
        da_s = eng._drop(pn + "attn", cfg.attention_probs_dropout_prob, train)
        da_p = eng._drop(pn + "attn.private", cfg.attention_probs_dropout_prob, train)
        lse_s = torch.empty((G, heads, T), dtype=F32, device=dev) if save else None
        lse_p = torch.empty((B, heads, W), dtype=F32, device=dev) if save else None
        s_var, p_var, p_mask, p_ks = (s_off, s_len), (p_off, p_len), (pwords, nw, W * nw), (ks_off, ks_len, 1)
        eng._attn_rows(q, k, v, ctx, (ones_t, 0, nw), G, heads, T, T, D, qvar=s_var, kvar=s_var, **train_kw(da_s, lse_s))
        eng._attn_rows(q, k, v, ctx, p_mask, B, heads, W, T, D, qvar=(p_off, p_len, None, p_ord), kvar=p_var, kshared=p_ks,
                       **train_kw(da_p, lse_p))
        x2_32, x2, post_bwd = eng._post_attn(eng._ctx_operand(ctx), x32, so, ff1, ff2, key + ".ln1", key + ".ln2",
                                             eng._drop(pn + "so", cfg.hidden_dropout_prob, train),
                                             eng._drop(pn + "out", cfg.hidden_dropout_prob, train), save)
        if save:
            def bwd(dx2):
                dctx, dpre1 = post_bwd(dx2)
                dqkv = eng._qkv_grad(qkv)                          # every row is written: S rows by the first launch, P rows by the second
                dq, dk, dv = dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:3 * H]
                eng._attn_bwd(q, k, v, ctx, dctx, lse_s, (ones_t, 0, nw), dq, dk, dv, 3 * H, G, heads, T, T, D, da_s, qvar=s_var, kvar=s_var)
                eng._attn_spliced_bwd(q, k, v, ctx, dctx, lse_p, p_mask, dq, dk, dv, B, heads, W, T, D, da_p, p_var, p_var, p_ks, groups_dev)
                return eng._proj_bwd(dqkv, x, qkv_l, dpre1)
            tape.append(("t", key, bwd))
        return x2_32, x2

    def conn_block(key, i, xv32, xv, xt32, xt):
        """BertConnectionLayer (models/vilbert_dialog.py:655-783): the image half once per group."""
        pn = f"bert.encoder.c_layer.{i}."
        lq1, lq2, d1, d2 = (eng.lin[key + s] for s in (".qkv1", ".qkv2", ".d1", ".d2"))
        vff1, vff2, tff1, tff2 = (eng.lin[key + s] for s in (".vff1", ".vff2", ".tff1", ".tff2"))
        da1 = eng._drop(pn + "attn1", cfg.v_attention_probs_dropout_prob, train)
        da2 = eng._drop(pn + "attn2", cfg.attention_probs_dropout_prob, train)
        db1 = eng._drop(pn + "bo1", cfg.v_hidden_dropout_prob, train)
        db2 = eng._drop(pn + "bo2", cfg.hidden_dropout_prob, train)
        dvo = eng._drop(pn + "vout", cfg.v_hidden_dropout_prob, train)
        dto = eng._drop(pn + "tout", cfg.hidden_dropout_prob, train)
        lse_v = torch.empty((G, nh, R), dtype=F32, device=dev) if save else None
        lse_t = torch.empty((G + B, nh, T), dtype=F32, device=dev) if save else None
        co_mask, v_mask, t_var, s_var = (ones_t, 0, nw), (it_vwords, 0, nwv), (it_off, it_len), (s_off, s_len)
        with eng._img():
            qkv1 = eng._proj(xv, lq1)
        qkv2 = eng._proj(xt, lq2)
        eng._to_txt(qkv1)
        eng._to_img(qkv2)
        if cache is not None:
            cache[key] = qkv1
        q1, k1, v1 = qkv1[:, :Hb], qkv1[:, Hb:2 * Hb], qkv1[:, 2 * Hb:]
        q2, k2, v2 = qkv2[:, :Hb], qkv2[:, Hb:2 * Hb], qkv2[:, 2 * Hb:]
        with eng._img():
            ctx_v = eng._ctx_rows(G * R, Hb, dev)
            # regions attend text (:701-721): the co-attention mask is 1 on the context [1, c) = all of S_g
            eng._attn_rows(q1, k2, v2, ctx_v, co_mask, G, nh, R, T, Db, kvar=s_var, **train_kw(da2, lse_v))
            ov32, ov, bwd_v = eng._post_attn(eng._ctx_operand(ctx_v), xv32, d1, vff1, vff2, key + ".lnb1", key + ".lnv", db1, dvo, save)
        ctx_t = eng._ctx_rows(M, Hb, dev)
        # text attends regions (:681-698): every packed text block against its group's regions
        eng._attn_rows(q2, k1, v1, ctx_t, v_mask, G + B, nh, T, R, Db, qvar=t_var, kvar=(it_koff, it_klen), **train_kw(da1, lse_t))
        ot32, ot, bwd_t = eng._post_attn(eng._ctx_operand(ctx_t), xt32, d2, tff1, tff2, key + ".lnb2", key + ".lnt", db2, dto, save)
        if save:
            def bwd(dov, dot):
                with eng._img():
                    dqkv1 = eng._qkv_grad(qkv1)
                dqkv2 = torch.zeros_like(qkv2)                     # (no region attends a P row: its K2 / V2 gradient is zero)
                eng._to_txt(dqkv1)
                eng._to_img(dqkv2)
                with eng._img():
                    dctx_v, dprev = bwd_v(dov)
                    eng._attn_bwd(q1, k2, v2, ctx_v, dctx_v, lse_v, co_mask, dqkv1[:, :Hb], dqkv2[:, Hb:2 * Hb], dqkv2[:, 2 * Hb:3 * Hb],
                                  3 * Hb, G, nh, R, T, Db, da2, kvar=s_var)
                dctx_t, dpret = bwd_t(dot)
                # one copy of its group's region K / V per text block, one dK / dV copy back, then the groups' sums in list order
                rep1 = torch.empty(((G + B) * R, 3 * Hb), dtype=BF16, device=dev)
                L.gather_rows(qkv1, rep_rows, rep1, (G + B) * R, 3 * Hb)
                dkv = torch.empty(((G + B) * R, 2 * Hb), dtype=BF16, device=dev)
                eng._attn_bwd(q2, rep1[:, Hb:2 * Hb], rep1[:, 2 * Hb:], ctx_t, dctx_t, lse_t, v_mask, dqkv2[:, :Hb], dkv[:, :Hb], dkv[:, Hb:],
                              2 * Hb, G + B, nh, T, R, Db, da1, qvar=t_var, kvar=(rep_koff, it_klen))
                L.segment_rows_sum_bf16(dkv, it_first, it_seq, dqkv1[:, Hb:], R, 2 * Hb)
                eng._to_img()                                      # dK1 / dV1 written by the text side
                eng._to_txt()                                      # dK2 / dV2 written by the image side
                with eng._img():
                    dxv = eng._proj_bwd(dqkv1, xv, lq1, dprev)
                dxt = eng._proj_bwd(dqkv2, xt, lq2, dpret)
                return dxv, dxt
            tape.append(("c", key, bwd))
        return ov32, ov, ot32, ot

    # ---- encoder (schedule of models/vilbert_dialog.py:842-929) ---------------------------------------------------------
    for kind, i in PM.encoder_schedule(cfg):
        if kind == "v":
            with eng._img():
                xv32, xv = eng._self_block(f"v{i}", xv32, xv, vmask, G, R, cfg.v_num_attention_heads, f"bert.encoder.v_layer.{i}.",
                                           cfg.v_attention_probs_dropout_prob, cfg.v_hidden_dropout_prob, st)
            if save:
                tape[-1] = ("v", tape[-1][0], tape[-1][1])
        elif kind == "t":
            xt32, xt = text_block(f"t{i}", i, xt32, xt)
        else:
            with eng._conn_tag():
                xv32, xv, xt32, xt = conn_block(f"c{i}", i, xv32, xv, xt32, xt)
    eng._to_txt(xv32, xv)

    out = dict(plan=plan, ok=same)
    if cache is not None:
        cache["vwords"] = vmask[0].view(G, nwv)
    # ---- poolers + NSP (models/vilbert_dialog.py:946-967, 1064-1070): row 0 of every sequence, region 0 of its group -------
    if want_nsp:
        xt32d, xv32d = eng._dense32(xt32), eng._dense32(xv32)
        out["nsp"] = eng._pooled_heads(xt32d, xv32d, p_off, (gid * R).to(torch.int32), B, False)["nsp_pad"][:, :2]
    # ---- MLM head on the copy rows (:982-986, :1023-1026) ------------------------------------------------------------------
    n = plan.n_lm
    lm_idx = _i32(plan.lm_idx, dev)
    lm_pos = _i64(plan.lm_pos, dev)
    lab_sel = lab_d.reshape(-1)[lm_pos].to(torch.int32)
    lmw = inp.get("lm_weight") if save else None
    w_sel = (torch.ones(n, dtype=torch.int32, device=dev) if lmw is None else
             lmw.to(dev, non_blocking=True).reshape(-1)[lm_pos].to(torch.int32))
    xs = torch.empty((n, xt.shape[1]), dtype=BF16, device=dev)             # rows of the GEMM operand: H, or the split's 3 H, bf16 words
    L.gather_rows(xt, lm_idx, xs, n, xt.shape[1])
    if save:
        lm = eng._lm_head(xs, n, lab_sel, w_sel, True, objective=inp.pop(LO.KEY, LO.LIKELIHOOD), pos=lm_pos.to(torch.int32))
        lm.update(n=n, idx=lm_idx)
        out["lm"], out["bwd"] = lm, dict(tape=tape, embt=bwd_embt, embv=bwd_embv)
    else:
        lm = eng._lm_head(xs, n, lab_sel, w_sel, False)
    out["rownll"] = lm["rownll"]
    if cache is not None or want_logits:
        out["logits"] = lm["logits"]
    out["lm_seq"] = (lm_pos // T).to(torch.int32)
    return out


def sequence_log_likelihood_shared(model, input_ids, image_feat, image_loc, masked_lm_labels, shared_context, average=False, **kw):
    """Drop-in for BertForMultiModalPreTraining.sequence_log_likelihood when the caller knows which sequences share their
    dialog context and image (`shared_context`: one group id per sequence -- the round index of val_lm.py's
    [rounds, options] batch -- or a `SharedContext` of them, which admits candidates of up to 30 tokens).  Returns (scores [B] fp32, nsp [B, 2]); sequences whose context turns out NOT to match their
    group's first member come back as NaN."""
    eng = model._engine
    eng.ensure(model._device())
    inp = dict(input_ids=input_ids, image_feat=image_feat, image_loc=image_loc, masked_lm_labels=masked_lm_labels, **kw)
    # CPU tensors (val_lm.py:86-121 passes them chunk by chunk) through the engine's staging ring; the text masks packed on the host,
    # the [B, R] image key mask as a tensor (this path indexes it by group)
    eng.stage_host_inputs(inp, pack=("attention_mask", "co_attention_mask"))
    out = forward_shared(eng, inp, shared_context)
    B = input_ids.shape[0]
    scores = torch.zeros(B, dtype=torch.float32, device=eng.arena.device)
    n = out["plan"].n_lm
    L.segment_sum(out["rownll"], out["lm_seq"], scores, n, -1.0)
    if average:
        cnt = torch.from_numpy(out["plan"].n.astype(np.float32)).to(scores.device)
        scores = scores / cnt
    scores = torch.where(out["ok"], scores, torch.full_like(scores, float("nan")))
    return scores, out.get("nsp")


def check_shared_training(cfg, compute_dtype, loss_weights, attention_mask, groups, T, R):
    """What `forward_backward(shared_context=...)` refuses, on the host, before anything reaches the device."""
    c_lm, c_nsp, c_img = (float(c) for c in loss_weights)
    if c_nsp != 0.0 or c_img != 0.0:
        raise ValueError(f"shared_context trains the LM term only: loss_weights must be (c, 0, 0), got {tuple(loss_weights)}")
    if compute_dtype != "bf16":
        raise ValueError(f"the shared-context training step runs on the bf16 engine only (compute_dtype={compute_dtype!r})")
    if not cfg.with_coattention or cfg.fixed_t_layer or cfg.fixed_v_layer:
        raise ValueError("the shared-context training step needs the connection layers (with_coattention) and no frozen layers "
                         "(fixed_t_layer = fixed_v_layer = 0)")
    check_shared_head_size(cfg, "shared_context training")
    spec = attention_mask
    if not isinstance(spec, DialogMaskSpec) or len(spec) == 0 or int(spec.mode.min()) != 1:
        raise ValueError("shared_context: attention_mask must be a generative-mode DialogMaskSpec (one descriptor per sequence)")
    n = spec.answer.astype(np.int64)
    length = spec.length.astype(np.int64) + n
    return SharedContextPlan(groups, length - 2 * n, n, length, T, R)


def train_shared(eng, inp, groups, g_lm, train):
    """Forward and backward of the LM term on the shared schedule -> the LM loss (fp32 [1]).  `ok` -- every sequence's context,
    image and labels are its group's -- stays on the device: it multiplies the loss gradient (a mismatch adds nothing to the
    gradient arena) and turns the returned loss into NaN.  g_lm None: the forward and the loss alone, no backward."""
    dev = eng.arena.device
    cfg = eng.cfg
    out = _forward_shared(eng, inp, groups, False, None, dict(train=train, tape=[]))
    lm, plan = out["lm"], out["plan"]
    n = lm["n"]
    ok = out["ok"].all().to(F32).reshape(1)
    lm_loss = lm["objective"].loss(eng, lm)                        # (this schedule's row count is the host's: no n_dev / inv_dev)
    if g_lm is None:
        return torch.where(ok > 0, lm_loss, torch.full_like(lm_loss, float("nan")))
    # ---- backward: the MLM head, then the tape (Engine._backward without poolers, NSP and image head)
    eng.arena.attach_grads()
    eng._bwd_fresh = bool(eng.arena.fresh)
    eng._ledger.begin()
    eng._step_rows = plan.M
    dxs = eng._transform_head_bwd(eng._lm_loss_grad(lm, g_lm.reshape(1) * ok), lm, lm["xs"], eng.lin["lmtr"], "lmtr", eng.lin["dec"],
                                  M=n, N=cfg.vocab_size)
    gt = torch.zeros((plan.M, cfg.hidden_size), dtype=eng.grad_dtype, device=dev)
    L.gather_rows(dxs, lm["idx"], gt, n, dxs.shape[1], scatter=True)
    gv = torch.zeros((plan.G * plan.R, cfg.v_hidden_size), dtype=eng.grad_dtype, device=dev)
    eng._bucket_done("heads")
    eng._to_img(gv)
    eng._backward_encoder(out["bwd"], list(reversed(out["bwd"]["tape"])), gt, gv)
    eng._to_txt()
    eng._bucket_done("text_embeddings")
    eng.arena.fresh = False
    eng._bwd_fresh = False
    return torch.where(ok > 0, lm_loss, torch.full_like(lm_loss, float("nan")))
