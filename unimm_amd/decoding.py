"""The decode side of answer generation: one model's prefill, caches and decode step, shared by the plain call (beams or samples,
`generation._generate`) and by both models of a speculative call (`speculative.speculate`).

A side prefills G dialogs once (`context [SEP] [MASK]` through the shared-context pass of `scoring.py`, which keeps every text
layer's context K / V and every connection layer's region K1 / V1; its decoded row is copy row 0) and owns S = G * slots
hypothesis slots, slot s = g * slots + j reading dialog g's context, each with a private cache of its answer rows' K | V in every
text layer (`priv` [text layers, S, pcap, 2 H], `plen` rows in use, double-buffered).  `rows` pushes P (answer row, copy row)
pairs per slot through the text side of the blocks -- the mask argument of `generation.py` is why nothing else has to run -- and
decodes the copy rows asked for.

The attention kernels take the slots in `groups` of `per_group` that share one context range, region range and key mask:
per_group = slots for the plain call (a dialog's beams or samples are one group, P = 1) and per_group = 1 for speculation (every
slot a group of its own, the dialog's ranges repeated per slot, so that per_group * 2 P <= 32 bounds the pairs whatever `slots`
is).  The side does not ask which: the kernels refuse per_group * 2 P > 32.

A step's new K | V rows (the fused projections every text layer leaves in the stash of its P) join the private caches in one of
three ways, each at the time its caller chooses: `reorder` (beams: children inherit their parent's rows, `unimm_kv_cache_update`
into a second buffer), `append_in_place` (samples: a slot keeps its own rows, a tensor assignment) and `append` (speculation: a
count of rows per slot, `unimm_kv_cache_append`).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import lib as L
from . import params as PM
from .inputs import DialogMaskSpec

SEP, MASK = 102, 103
BF16, F32 = torch.bfloat16, torch.float32


def answer_ids(pos_last, seg_last, k):
    """(position id, segment id) of answer token k (and of its [MASK] copy) after a context whose last token has them."""
    return pos_last + 1 + k, seg_last ^ 1


class DecodeSide:
    """One model's side of a generation call (the module docstring).  limits: the dialogs' token limits; pcap: rows of a slot's
    private cache; banned: the banned ids on the device (`top1`), or None."""

    def __init__(self, eng, inp, c_h, limits, pcap, banned, slots, per_group):
        from .scoring import _forward_shared
        self.eng, cfg, dev = eng, eng.cfg, eng.arena.device
        self.cfg, self.dev = cfg, dev
        ids = inp["input_ids"].to(dev, non_blocking=True)
        G, T = ids.shape
        self.G, self.T, self.R = G, T, inp["image_feat"].shape[1]
        self.S, self.per_group, self.groups = G * slots, per_group, G * slots // per_group
        S = self.S
        ar = torch.arange(G, device=dev)
        c_d = torch.from_numpy(c_h).to(dev)
        tt = inp.get("token_type_ids")
        tt = tt.to(dev, non_blocking=True).long() if tt is not None else torch.zeros((G, T), dtype=torch.int64, device=dev)
        pp = inp.get("position_ids")
        pp = pp.to(dev, non_blocking=True).long() if pp is not None else torch.arange(T, device=dev).repeat(G, 1)
        pos0, seg0 = answer_ids(pp[ar, c_d - 1], tt[ar, c_d - 1], 0)
        # ---- prefill: `context [SEP] [MASK]` per dialog through the shared-context pass, keeping the caches ----------------
        pid, ptt, ppp = ids.long().clone(), tt.clone(), pp.clone()
        lab = torch.full((G, T), -1, dtype=torch.int64, device=dev)
        for j, tok in ((0, SEP), (1, MASK)):
            pid[ar, c_d + j] = tok
            ptt[ar, c_d + j] = seg0
            ppp[ar, c_d + j] = pos0
        lab[ar, c_d + 1] = SEP
        pin = dict(input_ids=pid, image_feat=inp["image_feat"], image_loc=inp["image_loc"], token_type_ids=ptt, position_ids=ppp,
                   masked_lm_labels=lab, attention_mask=DialogMaskSpec(np.ones(G), c_h + 1, np.ones(G)))
        for k in ("image_attention_mask", "image_index"):
            if k in inp:
                pin[k] = inp[k]
        self.cache = {}
        self.pre = _forward_shared(eng, pin, np.arange(G), False, self.cache)
        plan = self.pre["plan"]
        rep = lambda a, n: a.repeat_interleave(n, 0) if n > 1 else a     # noqa: E731
        self.slot_pos, self.slot_seg = rep(pos0, slots), rep(seg0, slots)
        self.limits = rep(torch.from_numpy(np.asarray(limits, dtype=np.int64)).to(dev), slots)
        ng = slots // per_group                                          # groups per dialog
        self.s_off, self.s_len = (rep(torch.from_numpy(a.astype(np.int32)).to(dev), ng) for a in (plan.s_off, plan.s_len))
        self.k_off = rep((ar * self.R).to(torch.int32), ng)
        self.k_len = torch.full((self.groups,), self.R, dtype=torch.int32, device=dev)
        self.vwords = rep(self.cache["vwords"], ng)
        self.sched = PM.encoder_schedule(cfg)
        tkeys = [f"t{i}" for kind, i in self.sched if kind == "t"]
        self.nt, self.lidx = len(tkeys), {key: n for n, key in enumerate(tkeys)}
        self.pcap, self.banned = pcap, banned
        self.priv = torch.zeros((self.nt, S, pcap, 2 * cfg.hidden_size), dtype=BF16, device=dev)
        self.spare = None                                                # `reorder`'s second buffer
        self.plen = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2)]
        self.cur = 0
        self.per_P = {}

    def _buffers(self, P):
        """What depends on the pairs per slot: the per-layer projection stash, the rows' segments, the connection layers' query
        ranges, the scratch of the top-1, the copy rows of each `decode` list seen."""
        if P not in self.per_P:
            S, dev, n = self.S, self.dev, 2 * P * self.per_group
            self.per_P[P] = dict(stash=torch.empty((self.nt, S * 2 * P, 3 * self.cfg.hidden_size), dtype=BF16, device=dev),
                                 typ=self.slot_seg.repeat_interleave(2 * P).to(torch.int32),
                                 q_off=(torch.arange(self.groups, device=dev) * n).to(torch.int32),
                                 q_len=torch.full((self.groups,), n, dtype=torch.int32, device=dev),
                                 vals=torch.empty((S * P, 1), dtype=F32, device=dev),
                                 tops=torch.empty((S * P, 1), dtype=torch.int32, device=dev), sel={})
        return self.per_P[P]

    def rows(self, tokens, k, decode):
        """tokens int64 [S, P]: the token of answer row k[s, j] - 1; k int64 [S, P]: the step of pair j's copy row (an int where
        every slot stands at the same step).  The slots' private rows are [0, plen[cur]).  decode: the pairs whose copy rows are
        decoded -> fp32 logits [S * len(decode), Vpad]."""
        eng, cfg, dev, S, groups = self.eng, self.cfg, self.dev, self.S, self.groups
        P = tokens.shape[1]
        M = S * 2 * P
        buf = self._buffers(P)
        H, Hb = cfg.hidden_size, cfg.bi_hidden_size
        heads, nh = cfg.num_attention_heads, cfg.bi_num_attention_heads
        D, Db = H // heads, Hb // nh
        NO = L.NO_DROP
        kc = self.limits[:, None].clamp(max=k)                              # rows past a dialog's limit are dropped: keep their ids inside
        ids32 = torch.stack([tokens, torch.full_like(tokens, MASK)], 2).reshape(M).to(torch.int32)
        pos32 = (self.slot_pos[:, None, None] + torch.stack([(kc - 1).clamp_min(0), kc], 2)).reshape(M).to(torch.int32)
        xt32, xt, _ = eng._embed_text(ids32, pos32, buf["typ"], M, None, NO, False, None)
        plen = self.plen[self.cur]
        attn = L.attn_decode if P == 1 else L.attn_verify
        for kind, i in self.sched:
            if kind == "t":
                key = f"t{i}"
                qkv_l, so, ff1, ff2 = (eng.lin[key + s] for s in (".qkv", ".so", ".ff1", ".ff2"))
                li = self.lidx[key]
                qkv = eng._linear(xt, qkv_l, out=buf["stash"][li])
                ctxq = self.cache[key]
                ctx = torch.empty((M, H), dtype=BF16, device=dev)
                pv = self.priv[li].view(S * self.pcap, 2 * H)
                attn(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], ctx, ctxq[:, H:2 * H], ctxq[:, 2 * H:], self.s_off, self.s_len,
                     pv[:, :H], pv[:, H:], plen, groups, self.per_group, 2 * P, heads, self.pcap, 1.0 / math.sqrt(D))
                xt32, xt = eng._post_attn(ctx, xt32, so, ff1, ff2, key + ".ln1", key + ".ln2", NO, NO, False)[:2]
            elif kind == "c":                                               # the text half: the regions never attend the answer
                key = f"c{i}"
                lq2, d2, tff1, tff2 = (eng.lin[key + s] for s in (".qkv2", ".d2", ".tff1", ".tff2"))
                qkv1 = self.cache[key]
                qkv2 = eng._linear(xt, lq2)
                ctx_t = torch.empty((M, Hb), dtype=BF16, device=dev)
                vwords = self.vwords
                L.attn_fwd(qkv2[:, :Hb], qkv1[:, Hb:2 * Hb], qkv1[:, 2 * Hb:], ctx_t, None, vwords, groups, nh, self.T, self.R, Db,
                           1.0 / math.sqrt(Db), 0, vwords.shape[1], NO, qvar=(buf["q_off"], buf["q_len"]),
                           kvar=(self.k_off, self.k_len))
                xt32, xt = eng._post_attn(ctx_t, xt32, d2, tff1, tff2, key + ".lnb2", key + ".lnt", NO, NO, False)[:2]
        n = S * len(decode)
        sel = buf["sel"].get(tuple(decode))
        if sel is None:
            sel = (torch.arange(S, device=dev)[:, None] * 2 * P + 2 * torch.as_tensor(decode, device=dev)[None] + 1).reshape(n)
            sel = buf["sel"][tuple(decode)] = sel.to(torch.int32)
        xs = torch.empty((n, H), dtype=BF16, device=dev)
        L.gather_rows(xt, sel, xs, n, H)
        return eng.decode_rows(xs, n)

    def top1(self, logits, rows, flags, P):
        """The greedy token of every row and its log p under the rows' flags (unimm_lm_topk, K = 1) -> (logp [rows], id [rows])."""
        buf = self._buffers(P)
        L.lm_topk(logits, rows, self.cfg.vocab_size, self.banned, flags.reshape(rows).contiguous(), SEP, 1, buf["vals"][:rows],
                  buf["tops"][:rows])
        return buf["vals"][:rows, 0], buf["tops"][:rows, 0]

    # ---- the three ways a step's answer rows join the private caches (P = 1 unless said) --------------------------------
    def reorder(self, parent):
        """Slot s continues slot parent[s]: its rows and the parent's answer row of the last `rows` call, into the other buffer."""
        cur, H, stash = self.cur, self.cfg.hidden_size, self._buffers(1)["stash"]
        if self.spare is None:
            self.spare = torch.zeros_like(self.priv)
        L.kv_cache_update(self.priv, self.spare, stash[0][:, H:], parent.to(torch.int32), self.plen[cur], self.plen[1 - cur],
                          self.nt, self.S, self.pcap, 2 * H, stash.shape[1] * 3 * H, 2)
        self.priv, self.spare, self.cur = self.spare, self.priv, 1 - cur

    def append_in_place(self, r):
        """Every slot keeps the answer row of the last `rows` call as its private row r."""
        self.priv[:, :, r] = self._buffers(1)["stash"][:, 0::2, self.cfg.hidden_size:]
        self.plen[self.cur].add_(1)

    def append(self, count, P):
        """Append the first count[s] answer rows the last `rows` call with P pairs pushed to the private cache of slot s."""
        cur, H = self.cur, self.cfg.hidden_size
        stash = self._buffers(P)["stash"]
        L.kv_cache_append(self.priv, stash[0][:, H:], count.to(torch.int32), self.plen[cur], self.plen[1 - cur], self.nt, self.S,
                          self.pcap, 2 * H, P, stash.shape[1] * 3 * H, 2 * P, 2)
        self.cur = 1 - cur
