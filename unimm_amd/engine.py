"""Hot-path engine: the explicit forward / backward schedule of the two-stream co-attention
transformer over the hand-written HIP kernels (unimm_amd.lib), with weights in a flat arena.

What the reference runs as ~600 eager torch ops per step through autograd
(models/vilbert_dialog.py:1359-1626) is here a fixed launch schedule:

  forward  : mask bit-pack -> text/image embeddings -> [T|V|C blocks in BertEncoder order] ->
             poolers/NSP, row-sparse MLM decoder + fused log-softmax/UL loss, region head + KL
  backward : the same blocks in reverse, each a handful of fused kernels; weight gradients are
             accumulated straight into the flat fp32 gradient arena.

Activations are bf16 [rows, hidden] row-major; GEMMs accumulate in fp32; LayerNorm statistics,
softmax, log-sum-exp and all loss arithmetic are fp32.  There is no CPU / eager fallback here: every
compute step is a C-ABI call and raises if the library is missing."""
from __future__ import annotations

import copy
import math
import os
import zlib
from collections import namedtuple
from contextlib import contextmanager
from typing import Dict, List, Optional

import torch

from . import bucket_plan as BP
from . import dropout as DR
from . import lib as L
from . import lm_objective as LO
from . import params as PM
from .arena import FlatArena
from .inputs import DialogMaskSpec, HostStager, PackedMask

BF16 = torch.bfloat16
F32 = torch.float32


def _site(name: str) -> int:
    return zlib.crc32(name.encode()) & 0xFFFFFFFF


def _rup(x, m):
    return (x + m - 1) // m * m


def _rows16(x):
    """-> (x as rows of 16-bit elements, their number per row): the row-moving kernels take fp32 rows as 2 H such elements"""
    return (x.view(BF16), 2 * x.shape[1]) if x.dtype == F32 else (x, x.shape[1])


# inputs that `stage_host_inputs` moves to the device (nsp_weight stays on the host: it is read there)
_STAGED_KEYS = ("input_ids", "token_type_ids", "position_ids", "masked_lm_labels", "lm_weight", "next_sentence_label", "image_label",
                "image_attention_mask", "attention_mask", "co_attention_mask", "image_loc", "image_feat", "image_target", "image_index")


class _LazyLN:
    """fp32 residual-stream value that is LayerNorm(x) but was never written: (x, mean, rstd, gamma, beta)."""
    __slots__ = ("x", "mean", "rstd", "gamma", "beta")

    def __init__(self, x, mean, rstd, gamma, beta):
        self.x, self.mean, self.rstd, self.gamma, self.beta = x, mean, rstd, gamma, beta


# One queued weight gradient dw[N,K] += dy[:M,:N]^T x[:M,:K], in the field order `lib.gemm_tn_grouped` takes
_WGrad = namedtuple("_WGrad", "dy x dw M N K dbias m_dev overwrite", defaults=(None, None, False))


class _Lin:
    """One (possibly fused) linear: bf16 weight [N,K], transposed bf16 copy [K,Npad], fp32 bias + grads."""
    __slots__ = ("w", "wt", "bias", "gw", "gb", "N", "K", "gbs")

    def __init__(self, w, wt, bias, gw, gb, gbs=None):
        self.w, self.wt, self.bias, self.gw, self.gb = w, wt, bias, gw, gb
        self.N, self.K = w.shape
        self.gbs = gbs  # extra bias-gradient destinations (image embedding: b_feat and b_loc)


class Engine:
    def __init__(self, model, cfg):
        self.model = model
        self.cfg = cfg
        self.arena: Optional[FlatArena] = None
        self.seed = 0x5EED
        self.step = 0
        self._w_version = None
        self.lin: Dict[str, _Lin] = {}
        self.ln: Dict[str, tuple] = {}
        self.grad_bucket_hook = None     # set by the data-parallel wrapper: f(group_name, more_follow_at_once)
        self._anchor = None
        self.last_seq_t = None
        for report in LO.REPORTS:        # last_lm_*: what the last step's LM objective reported (None until one has)
            setattr(self, report, None)
        self.unpad = True                # run the text stream on valid rows only (see the plan step of _forward)
        # Weight gradients wait for a grouped launch, per side (0 = text, 1 = image: inside `_img()`).  The ledger, shared with
        # the exchange planner, decides when a side is launched and which gradient buckets that completes; the operands wait here.
        self._ledger = BP.Ledger()
        self._wq, self._fq = [[], []], [[], []]   # queued _WGrad problems / column-partials reductions of LayerNorm backward calls
        # Schedule options are plain attributes (set them on `model.engine` before the first step; bench.py has flags for
        # the ones that are measured: --single-stream).  One environment switch: UNIMM_PRUNE_LAST_TEXT (see below).
        self.lazy_ln = True              # residual epilogues evaluate the previous LayerNorm instead of reading its fp32 output
        # The attention launches take their (sequence, head) items longest sequence first (unimm_attn_args.order, written by the
        # step's plan): the tail of a launch is then its shortest items.  5,691 / 5,732 -> 5,793 / 5,818 sequences/s at 240
        # sequences with the BATCH sorted that way (bench.py --order-by-length, alternating runs); same results either way.
        self.attn_longest_first = True
        # Option: grouped weight-gradient launches on a side stream (`wgrad_stream = True`): +1.8 % throughput in
        # interleaved runs (61.2 -> 60.1 ms) because the next block's GEMMs fill the partial last round and the
        # atomic drain.  Off by default: overlapped kernels stretch each other's durations, so per-kernel event /
        # rocprof timings (bench.py's roofline block) would no longer be exclusive.
        self.wgrad_stream = False
        self._side = None
        # Image-stream blocks on their own HIP stream (`dual_stream`, default on): between two connection layers the
        # image layer and the text layer are independent (models/vilbert_dialog.py:842-929), and the image side's
        # kernels are too small to fill 256 CUs (M = B*37 rows), so they run beside the text layer's and fill its
        # partial rounds; the same holds for the image half of a connection layer once the two co-attention
        # directions have exchanged their K/V.  Same kernels, same order within each stream.
        self.dual_stream = True
        self._text_stream = None      # the stream of the running engine entry (see _on_text_stream / _img)
        self._text_scope = None       # ... and the raw-stream object lib.stream_scope installed for it
        self._vside = None
        self.text_priority = False       # text side on an internal high-priority stream (measured -0.6 %: off)
        self._tstream = None
        self._on_side = False            # inside `_img()`: launches (and queued weight gradients) belong to the image side
        self.last_plan = None
        self._arena_users = []           # weakrefs of objects that cache `self.arena` (FusedAdamW, DataParallelRCCL)
        # Partial-tile workspaces of the weight-gradient launches, one per launch stream (text / image / optional side).
        # OFF by default (0 MB = every split adds its partial tile with fp32 atomics): the slab + last-arriver reducer
        # of unimm_gemm_tn_grouped_ws measured SLOWER at 240 sequences (4,797 against 4,949 sequences/s, interleaved
        # runs on one box; single problems 220 against 128 us): the last round's ~108 reducers each read 1.5 MB of
        # slabs serially and every split's agent-scope release writes back its XCD's L2.  `wgrad_ws_bytes = 512 << 20` enables it.
        self.wgrad_ws_bytes = 0
        self._wgrad_ws = {}
        self._plist = []
        self.gemm_tile = 0               # tuning code handed to every encoder GEMM (unimm_gemm_nt_args.tile; 0 = automatic)
        # Weight-gradient launches cover SEVERAL encoder blocks (see `_flush_wgrad`): a launch is due once its 256x256 tiles
        # fill about `wgrad_group_rounds` rounds of the chip; a data-parallel wrapper may lower it (smaller, earlier buckets).
        self.wgrad_group_rounds = 4
        # Row-count capacities.  Launch arguments hold CAPACITIES (the step's valid text rows / decoded rows rounded up to
        # these buckets); kernels whose result depends on the surplus rows read the real counts from the step's own device
        # words (`out["dyn"]`, written by unimm_plan_build; allocated per forward).  1 = exact sizes (default); the graph executor (unimm_amd/graphs.py) raises them
        # so that steps with nearby row counts replay one captured launch sequence.
        self.row_bucket, self.lm_bucket = 1, 1
        self.salt_word = None            # int32 [1] device tensor holding dropout.step_salt(seed, step), or None (see _drop)
        self._inject_header = None       # header values of the step, read ahead of a graph capture (see _forward, graphs.py)
        self.graphs = None               # unimm_amd.graphs.StepGraphs once enable_graphs() was called
        self.image_tile = 0              # tile code of the image side's GEMMs in the large-batch regime (0 = the library's choice; see _tile)
        self.wgrad_overwrite = True      # weight gradients with a single contributor are WRITTEN into a freshly zeroed arena (no atomics)
        self._bwd_fresh = False
        self.debug_fresh = False         # check (one device scan + sync per backward) that a `fresh` arena really is zero
        self.tile_table = {}             # {("t" | "i", N, K): tile code}: per-shape choices of the small-batch regime (see _tile)
        self.small_rows = 12000          # text rows per step below which the encoder GEMMs take the small-batch tile rule (_tile)
        self._step_rows = None           # text rows of the running step (set by _forward)
        self.image_head_side = True      # image prediction head (forward and backward) on the image stream, beside the MLM head
        self.attn_sink = None            # dict while a forward collects attention probabilities (forward_with_attention)
        self.skinny_dx_rows = 3072       # decoded-row count up to which the decoder's input gradient runs as a split reduction (_decoder_dx)
        self.prof_conn = None            # bench.py: dict while the launch profiler tags the connection layers' GEMMs (see _conn_tag)
        # Split-K for the long reductions of the small-batch regime (see _splitk): workspace per launch stream, zero-filled once
        self.splitk = True
        self.splitk_ws_bytes = 48 << 20
        self._splitk_ws = {}
        self.host_staging = True         # CPU tensors handed to forward() go through a pinned staging ring + copy stream (stage_host_inputs)
        self._stager = None
        # The last text layer feeds nothing but the MLM head (on the labelled rows) and the text pooler (on the first-token
        # rows).  In a training step whose caller wants no sequence output, the row-wise half of that layer -- everything after
        # the attention (`_post_attn`) -- and the heads therefore run on those rows alone, B first-token rows followed by the
        # plan's labelled rows (~17 % of the rows at 240 sequences); the rows keep the dropout masks of the rows they came from
        # (unimm_gemm_nt_args.drop_rows).  See `_prune_rows`.  UNIMM_PRUNE_LAST_TEXT=0 (read here, for A/B runs of bench.py)
        # or `prune_last_text = False` runs the layer on all rows.
        self.prune_last_text = os.environ.get("UNIMM_PRUNE_LAST_TEXT", "1") != "0"
        self._seq_wanted = True          # the running forward's caller reads the text stream's sequence output (see forward)

    def __deepcopy__(self, memo):
        """A copied model (policy.frozen_reference) gets an engine of its own: bound to the copy, with this engine's dropout
        seed / step, and EMPTY -- arena, weight copies, streams and staging ring are built at its first forward."""
        model = memo.get(id(self.model))
        if model is None:
            raise TypeError("an Engine is copied with its model: copy.deepcopy(model)")
        new = type(self)(model, copy.deepcopy(self.cfg, memo))
        new.seed, new.step = self.seed, self.step
        return new

    def schedule_key(self):
        """Every schedule attribute that is frozen into a captured launch sequence (unimm_amd/graphs.py keys its entries on
        it: changing one after a capture re-captures instead of replaying the old schedule beside an eager new one)."""
        return (self.dual_stream, self.unpad, self.lazy_ln, self.gemm_tile, self.wgrad_group_rounds, self.wgrad_stream, self.splitk,
                self.attn_longest_first, self.wgrad_overwrite, tuple(sorted(self.tile_table.items())), self.image_tile,
                self.small_rows, self.image_head_side, self.skinny_dx_rows, self.wgrad_ws_bytes, self.text_priority,
                self.prune_last_text)

    def register_arena_user(self, obj):
        import weakref
        self._arena_users.append(weakref.ref(obj))

    # ------------------------------------------------------------------------------------------
    # arenas + bf16 weight copies
    # ------------------------------------------------------------------------------------------
    def ensure(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise L.UnimmHipError("unimm_amd runs on the GPU only (gfx950); move the model with .cuda() first")
        L.lib()
        if self.arena is not None and self.arena.is_current() and self.arena.device == device:
            return
        if self.arena is not None:
            users = [u() for u in self._arena_users]
            users = [type(u).__name__ for u in users if u is not None]
            if users:
                raise L.UnimmHipError(
                    "the model's parameters were re-pointed (module.to(), load_state_dict(assign=True), a replaced "
                    f"Parameter) while {', '.join(users)} still hold the engine's flat arena: build the optimizer / "
                    "data-parallel wrapper after the model has reached its final device")
        self.cfg.validate_for_hip()
        named = {n: p for n, p in self.model.named_parameters()}   # tied decoder alias is deduplicated
        self.arena = FlatArena(named, PM.arena_groups(self.cfg), device=device, no_grad=PM.no_grad_names(self.cfg))
        A = self.arena
        self.w16 = torch.zeros(A.numel, dtype=BF16, device=device)
        self._anchor = torch.zeros(1, device=device, requires_grad=True)
        self._plist = list(named.values())
        self._build_tables(device)
        self._w_version = None
        self._wt_table = None

    def invalidate_weights(self):
        """The fp32 master weights changed behind the engine's back (load_state_dict, a broadcast, a raw-pointer
        write): the next forward re-casts the bf16 copies and rebuilds the transposed ones."""
        self._w_version = None

    def _weight_version(self):
        """Changes whenever a parameter (or the flat arena) was written through torch.  The Parameters are views
        created with `p.data = view`, so each has its OWN version counter: `p.copy_()`, `load_state_dict` and eager
        optimizers bump those, not `flat._version`.  Writes torch cannot see (`p.data.mul_()`, kernels taking raw
        pointers) need `invalidate_weights()`; the fused AdamW step refreshes the copies itself."""
        v = self.arena.flat._version
        for p in self._plist:
            v += p._version
        return v

    def _fused(self, names):
        """bf16 / fp32 / grad views spanning several consecutive arena entries (fused QKV)."""
        A = self.arena
        o0, shape0 = A.offsets[names[0]]
        rows = sum(A.offsets[n][1][0] for n in names)
        tail = shape0[1:]
        n_el = rows * (tail[0] if tail else 1)
        shp = (rows,) + tail
        # consecutive entries must be gap-free for the fused view to be valid
        o = o0
        for n in names:
            oo, s = A.offsets[n]
            assert oo == o, f"arena layout: {n} not contiguous"
            o += s[0] * (s[1] if len(s) > 1 else 1)
        return (self.w16[o0:o0 + n_el].view(shp), A.flat[o0:o0 + n_el].view(shp), A.grad_flat[o0:o0 + n_el].view(shp))

    def _mk_lin(self, key, wnames, bnames, device, kpad=None, make_wt=True):
        w16, _, gw = self._fused(wnames)
        _, b32, gb = self._fused(bnames) if bnames else (None, None, None)
        N, K = w16.shape
        wt = None
        if make_wt:
            wt = torch.zeros((K, kpad or _rup(N, 64)), dtype=BF16, device=device)
        self.lin[key] = _Lin(w16, wt, b32, gw, gb)
        self._wt_src.append((key, wnames))

    def _build_tables(self, device):
        cfg, A = self.cfg, self.arena
        self.lin.clear(); self.ln.clear()
        self._wt_src = []

        def ln(key, name):
            self.ln[key] = (A.view(name + ".weight"), A.view(name + ".bias"), A.grad(name + ".weight"), A.grad(name + ".bias"))

        def self_block(k, p):
            a = p + "attention.self."
            self._mk_lin(k + ".qkv", [a + n + ".weight" for n in ("query", "key", "value")],
                         [a + n + ".bias" for n in ("query", "key", "value")], device)
            self._mk_lin(k + ".so", [p + "attention.output.dense.weight"], [p + "attention.output.dense.bias"], device)
            ln(k + ".ln1", p + "attention.output.LayerNorm")
            self._mk_lin(k + ".ff1", [p + "intermediate.dense.weight"], [p + "intermediate.dense.bias"], device)
            self._mk_lin(k + ".ff2", [p + "output.dense.weight"], [p + "output.dense.bias"], device)
            ln(k + ".ln2", p + "output.LayerNorm")

        for kind, i in PM.encoder_schedule(cfg):
            if kind == "t":
                self_block(f"t{i}", f"bert.encoder.layer.{i}.")
            elif kind == "v":
                self_block(f"v{i}", f"bert.encoder.v_layer.{i}.")
            else:
                p = f"bert.encoder.c_layer.{i}."
                b = p + "biattention."
                k = f"c{i}"
                self._mk_lin(k + ".qkv1", [b + n + ".weight" for n in ("query1", "key1", "value1")],
                             [b + n + ".bias" for n in ("query1", "key1", "value1")], device)
                self._mk_lin(k + ".qkv2", [b + n + ".weight" for n in ("query2", "key2", "value2")],
                             [b + n + ".bias" for n in ("query2", "key2", "value2")], device)
                o = p + "biOutput."
                self._mk_lin(k + ".d1", [o + "dense1.weight"], [o + "dense1.bias"], device)
                ln(k + ".lnb1", o + "LayerNorm1")
                self._mk_lin(k + ".d2", [o + "dense2.weight"], [o + "dense2.bias"], device)
                ln(k + ".lnb2", o + "LayerNorm2")
                self._mk_lin(k + ".vff1", [p + "v_intermediate.dense.weight"], [p + "v_intermediate.dense.bias"], device)
                self._mk_lin(k + ".vff2", [p + "v_output.dense.weight"], [p + "v_output.dense.bias"], device)
                ln(k + ".lnv", p + "v_output.LayerNorm")
                self._mk_lin(k + ".tff1", [p + "t_intermediate.dense.weight"], [p + "t_intermediate.dense.bias"], device)
                self._mk_lin(k + ".tff2", [p + "t_output.dense.weight"], [p + "t_output.dense.bias"], device)
                ln(k + ".lnt", p + "t_output.LayerNorm")

        ln("emb_t", "bert.embeddings.LayerNorm")
        ln("emb_v", "bert.v_embeddings.LayerNorm")
        # poolers and the NSP head run in fp32 (unimm_linear_f32): fp32 master weight / bias and their gradient views
        self.lin32 = {k: (A.view(n + ".weight"), A.view(n + ".bias"), A.grad(n + ".weight"), A.grad(n + ".bias"))
                      for k, n in (("tpool", "bert.t_pooler.dense"), ("vpool", "bert.v_pooler.dense"),
                                   ("nsp", "cls.bi_seq_relationship"))}
        self._mk_lin("lmtr", ["cls.predictions.transform.dense.weight"], ["cls.predictions.transform.dense.bias"], device)
        ln("lmtr", "cls.predictions.transform.LayerNorm")
        self._mk_lin("dec", [PM.WORD_EMB], None, device)
        d = self.lin["dec"]
        d.bias, d.gb = A.view("cls.predictions.bias"), A.grad("cls.predictions.bias")
        self._mk_lin("imgtr", ["cls.imagePredictions.transform.dense.weight"],
                     ["cls.imagePredictions.transform.dense.bias"], device)
        ln("imgtr", "cls.imagePredictions.transform.LayerNorm")
        self._mk_lin("imgdec", ["cls.imagePredictions.decoder.weight"], ["cls.imagePredictions.decoder.bias"], device)
        # image embedding: one GEMM over [feat | loc | 0] with W_cat = [W_feat | W_loc | 0], bias = b_feat + b_loc
        F = cfg.v_feature_size
        self.vemb_k = F + 64
        self.vemb_w = torch.zeros((cfg.v_hidden_size, self.vemb_k), dtype=BF16, device=device)
        self.vemb_b = torch.zeros(cfg.v_hidden_size, dtype=F32, device=device)
        # embedding tables: gathered from the fp32 master weights
        e = "bert.embeddings."
        self.tab = {k: A.view(e + n + ".weight") for k, n in
                    (("word", "word_embeddings"), ("pos", "position_embeddings"), ("type", "token_type_embeddings"),
                     ("ext", "token_type_embeddings_extension"))}
        # column-partials scratch of the non-deferred LayerNorm / embedding backward calls: one set per stream (with
        # hidden_size == v_hidden_size the image stream's `bwd_embv` and the text stream's `bwd_embt` would otherwise
        # share one buffer without any ordering between them)
        self.part = {h: torch.empty(L.colpartials_bytes(h) // 4, dtype=F32, device=device)
                     for h in {cfg.hidden_size, cfg.v_hidden_size}}
        self.part_side = {h: torch.empty(L.colpartials_bytes(h) // 4, dtype=F32, device=device)
                          for h in {cfg.hidden_size, cfg.v_hidden_size}}

    def refresh_weights(self, force=False, cast=True):
        """fp32 arena -> bf16 copies (one cast kernel) + transposed copies for the dgrad GEMMs.
        cast=False: the caller (the fused AdamW step) has already written the bf16 copy."""
        A = self.arena
        ver = self._weight_version()
        if not force and ver == self._w_version:
            return
        if cast:
            L.cast_f32_bf16(A.flat, self.w16, A.numel)
        if self._wt_table is None:          # one descriptor table for every transposed copy, built once
            ents = []
            for key, wnames in self._wt_src:
                lin = self.lin[key]
                if lin.wt is None:
                    continue
                o0, _ = A.offsets[wnames[0]]
                ents.append((A.flat[o0:o0 + lin.N * lin.K].view(lin.N, lin.K), lin.wt))
            self._wt_table = L.transpose_table(ents, A.flat.device)
        L.transpose_cast_grouped(*self._wt_table)
        cfg = self.cfg
        F = cfg.v_feature_size
        v = "bert.v_embeddings."
        self.vemb_w[:, :F].copy_(A.view(v + "image_embeddings.weight"))
        self.vemb_w[:, F:F + 5].copy_(A.view(v + "image_location_embeddings.weight"))
        torch.add(A.view(v + "image_embeddings.bias"), A.view(v + "image_location_embeddings.bias"), out=self.vemb_b)
        self._w_version = ver

    # ------------------------------------------------------------------------------------------
    # small op helpers (each returns its output and pushes its backward onto the tape)
    # ------------------------------------------------------------------------------------------
    def _drop(self, name, p, train):
        """Dropout triple of one site.  Eagerly the key carries seed, step and site; with `salt_word` set (the graph
        executor) the argument is the per-site key and the per-step salt is read from that device word at kernel entry:
        the same masks either way (dropout.make_key = site_key ^ step_salt)."""
        if not train or p <= 0.0:
            return L.NO_DROP
        if self.salt_word is not None:
            return DR.drop_arg(p, DR.site_key(self.seed, _site(name))) + (self.salt_word,)
        return DR.drop_arg(p, DR.make_key(self.seed, self.step, _site(name)))

    def _linear(self, x, lin, epi=L.EPI_BIAS, aux=None, want_u=False, drop=None, out_f32=False, ldo=None, M=None, out=None,
                drop_rows=None, aux_rows=None):
        """drop_rows / aux_rows (EPI_BIAS_DROP_RESID): x holds a subset of rows; row m draws the dropout mask of row drop_rows[m]
        and reads its residual `aux` at row aux_rows[m]."""
        M = x.shape[0] if M is None else M
        ldo = ldo or lin.N
        if out is None:                              # or a caller's [M, ldo] buffer (answer generation's per-layer K / V stash)
            out = torch.empty((M, ldo), dtype=F32 if out_f32 else BF16, device=x.device)
        u = torch.empty((M, ldo), dtype=BF16, device=x.device) if want_u else None
        aux_ln = None
        if isinstance(aux, _LazyLN):
            aux, aux_ln = aux.x, (aux.mean, aux.rstd, aux.gamma, aux.beta)
        sk = self._splitk(M, lin.N, lin.K)
        if sk is not None:
            L.gemm_nt(x, lin.w, out, bias=lin.bias, epilogue=epi, aux=aux, out2=u, drop=drop, M=M, N=lin.N, K=lin.K, aux_ln=aux_ln,
                      tile=sk[0], splitk=sk[1], splitk_ws=sk[2], drop_rows=drop_rows, aux_rows=aux_rows)
        else:
            L.gemm_nt(x, lin.w, out, bias=lin.bias, epilogue=epi, aux=aux, out2=u, drop=drop, M=M, N=lin.N, K=lin.K, aux_ln=aux_ln,
                      tile=self._tile(M, lin.N, lin.K), drop_rows=drop_rows, aux_rows=aux_rows)
        return (out, u) if want_u else out

    def _tile(self, M, N, K=None):
        """Tile code of one encoder GEMM (unimm_gemm_nt_args.tile).  0 = the kernel library's own choice, which is tuned for
        launches that have the chip to themselves.  In the small-batch regime (fewer than `small_rows` text rows in the step: the
        per-GPU share of a batch split over 4-8 ranks) neither stream's launches fill the chip and the two streams' kernels run
        side by side all the time; there the 128x128 tile (64 KiB of LDS, two workgroups per CU, 15 KiB staged per MFLOP) beats
        both the one-per-CU tiles (112-128 KiB of LDS: nothing of the other stream fits beside them) and, on the image side,
        the 64x128 tile (twice the workgroups, 23 KiB per MFLOP): +3 % at 60 sequences; the text side's N = 768 GEMMs at ~4k rows
        (fewer than 256 tiles of 128x128) stay on 64x128 (-1.7 % otherwise at 30 sequences).
        In the large-batch regime the text side's launches fill the chip with one-per-CU workgroups, and what the image side's
        launches (M = 37 rows per sequence: a fraction of a round) cost the step is the CUs they keep from the text side: in
        rounds 3-4 the 256x256 ping-pong tile (140 CUs per image GEMM instead of 188) was +0.8 % at 240 sequences; with the
        three-slot X ring of round 5 the library's own 192x256 choice is back in front (+0.3 %, two alternating pairs), so
        `image_tile` is 0 again."""
        if self.gemm_tile != 0:                   # an explicit tuning code reaches both sides (A/B runs: bench.py --gemm-tile)
            return self.gemm_tile
        if self._step_rows is None:               # outside a step: the library's own choice
            return 0
        if self.tile_table and K is not None:     # per-shape codes (side, N, K) of the small-batch regime (bench.py --tile-table)
            code = self.tile_table.get(("i" if self._on_side else "t", N, K))
            if code is not None and self._step_rows < self.small_rows:
                return code
        if self._step_rows >= self.small_rows:
            return self.image_tile if (self._on_side and self.image_tile) else 0
        if self._on_side:
            return 14                             # 128x128 with the X operand on a three-slot ring (round 5: +0.5 % at 30, +1 % at 60 over tile 1)
        t128 = ((M + 127) // 128) * ((N + 127) // 128)
        return 7 if t128 < 256 else 1

    def _splitk(self, M, N, K):
        """(tile code, splitk, workspace) of a long-reduction GEMM in the small-batch regime, or None.  At ~4k text rows a
        K = 2304 / 3072, N = 768 GEMM is 366 tiles of 64x128, each a 36-48 step chain, and stages 430 MB through the L2s (the W
        panel is re-read by 61 row tiles): 128x128 tiles halve the staged bytes but leave 186 workgroups for 256 CUs -- two
        workgroups per tile, each reducing half of K and meeting in a workspace (unimm_gemm_nt_args.splitk), get both: 30.3
        against 33.6 us alone (profiles/r4c_small_batch_gemm_microbench.txt)."""
        if not self.splitk or self._on_side or self.gemm_tile != 0 or self._step_rows is None or self._step_rows >= self.small_rows:
            return None
        if M != self._step_rows:      # the text stream's GEMMs only, whatever stream they run on (one-stream runs must round alike)
            return None
        if K < 2048 or N > 1024 or ((M + 127) // 128) * ((N + 127) // 128) > 256:
            return None
        return 1, 2, self._splitk_workspace()

    def _splitk_workspace(self):
        """The split-K workspace (slabs + zero-between-launches tickets) is private to launches of ONE stream: keyed by the
        stream the launch goes to (the caller's stream in eager steps, the capturing stream under graph capture), so a
        text-side GEMM issued from another stream can never share tickets with one in flight."""
        dev = self.arena.flat.device
        key = int(torch.cuda.current_stream(dev).cuda_stream)
        ws = self._splitk_ws.get(key)
        if ws is None:
            ws = self._splitk_ws[key] = torch.zeros(self.splitk_ws_bytes, dtype=torch.uint8, device=dev)
        return ws

    def _linear32(self, x, key, relu=False, out=None):
        """y = act(x W^T + b) in fp32 from the fp32 master weights (poolers, NSP head; models/vilbert_dialog.py:946-967, :1070)."""
        w32, b32 = self.lin32[key][:2]
        N, K = w32.shape
        M = x.shape[0]
        if out is None:
            out = torch.empty((M, N), dtype=F32, device=x.device)
        return L.linear_f32(x, w32, out, M, N, K, (x.stride(0), 1), (1, w32.stride(0)), bias=b32, relu=relu)

    def _linear32_bwd(self, dy, x, key):
        """dW += dy^T x, db += colsum(dy) (fp32 atomics into the gradient arena), returns dx = dy W; all fp32."""
        w32, _, gw, gb = self.lin32[key]
        N, K = w32.shape
        M = dy.shape[0]
        L.linear_f32(dy, x, gw, N, K, M, (1, dy.stride(0)), (x.stride(0), 1), accumulate=True, rowsum=gb)
        dx = torch.empty((M, K), dtype=F32, device=dy.device)
        return L.linear_f32(dy, w32, dx, M, K, N, (dy.stride(0), 1), (w32.stride(0), 1))

    def _wgrad(self, dy, x, gw, M, N, K, dbias=None, m_dev=None, sole=False, rule_M=None):
        """dW += dy^T x (+ bias gradient).  Nothing downstream in the backward chain reads a weight gradient,
        so the call is only queued; `_flush_wgrad` hands the list of SEVERAL encoder blocks to one grouped launch
        (the ledger says when).  dy / x stay referenced by the queue until then.
        sole: this call is the ONLY contribution to gw in a backward pass (every encoder nn.Linear; not the tied decoder /
        word-embedding matrix, not the three split-operand products of the fp32x3 mode).  When the gradient arena is also known
        to be zero (`arena.fresh`: zeroed since the last backward) the kernel then writes the tile with plain stores instead of
        256 KiB of memory-side atomics per workgroup (unimm_gemm_tn_args.overwrite).
        rule_M: the row count the flush rule counts this problem with, when it is not M: a block that runs on a
        subset of the step's rows (`_prune_rows`) keeps the step's row count there, so that grouped launches and bucket
        hand-overs fall where they always fell -- the subset's size differs between the ranks of a data-parallel step."""
        self._wq[self._on_side].append(_WGrad(dy, x, gw, M, N, K, dbias, m_dev, bool(sole and self._bwd_fresh and self.wgrad_overwrite)))
        self._ledger.queue(int(self._on_side), M if rule_M is None else rule_M, N, K)
        if self.prof_conn is not None:            # FLOPs of the weight gradients queued from inside / outside a connection layer
            self.prof_conn["tn_conn" if self.prof_conn["in"] else "tn_other"] += 2.0 * M * N * K

    def _colsum(self, part, blocks, H, dsts):
        """Queue the reduction of a LayerNorm backward's column partials into `dsts` for the side's next grouped launch."""
        self._fq[self._on_side].append((part, blocks, H, dsts))
        self._ledger.colsum(int(self._on_side))

    @contextmanager
    def _conn_tag(self):
        """While bench.py profiles (`prof_conn` is a dict): the GEMM launches issued inside the block carry tag 1 in the launch
        profiler and the weight gradients queued inside it are counted as connection-layer FLOPs -- `roofline.coattention_gemms`,
        the projections and FFNs of models/vilbert_dialog.py:655-783, forward and backward."""
        if self.prof_conn is None:
            yield
            return
        L.prof_tag(1)
        self.prof_conn["in"] = True
        try:
            yield
        finally:
            self.prof_conn["in"] = False
            L.prof_tag(0)

    def _ws(self, which):
        """Zero-initialised workspace of the weight-gradient launches of one stream (0 bytes = fp32-atomic path)."""
        if self.wgrad_ws_bytes <= 0:
            return None
        t = self._wgrad_ws.get(which)
        if t is None:
            t = self._wgrad_ws[which] = torch.zeros(self.wgrad_ws_bytes, dtype=torch.uint8, device=self.arena.flat.device)
        return t

    def _flush_wgrad(self, force=False, force_img=False, sides=None):
        """Launch the sides the ledger names: `sides` as `_bucket_done` got them from its mark, else the ledger's direct flush
        (all of them with force=True; force_img: the image side's whatever its size) for callers outside a backward.
        Why launches are grouped over blocks: DESIGN.md, "Weight-gradient launches are grouped over blocks"."""
        for side in self._ledger.flush(self.wgrad_group_rounds, self._on_side, force, force_img) if sides is None else sides:
            self._launch_wgrad(side)

    def _launch_wgrad(self, side):
        probs, sums = self._wq[side], self._fq[side]
        self._wq[side], self._fq[side] = [], []
        shared = self._dual()                     # the launches of this backward share the chip with the other stream's
        if side:
            with self._img():                     # image-side problems: operands were produced on that stream
                L.gemm_tn_grouped(probs, shared=shared, ws=self._ws("img"))
                L.colpartials_finish_grouped(sums)
            return
        L.colpartials_finish_grouped(sums)
        if not probs:
            return
        if not self.wgrad_stream:
            L.gemm_tn_grouped(probs, shared=shared, ws=self._ws("txt"))
            return
        # side stream: the grouped launch ends with a partial last round and a memory-side atomic drain during
        # which most CUs idle; the next block's input-gradient GEMMs can fill them
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.arena.flat.device)
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side), L.stream_scope(self._side):
            L.gemm_tn_grouped(probs, shared=shared, ws=self._ws("side"))
        for p in probs:                           # keep the caching allocator from recycling them early
            p.dy.record_stream(self._side)
            p.x.record_stream(self._side)

    def _join_wgrad(self):
        if self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)

    def _linear_bwd(self, dy, x, lin, epi=L.EPI_BIAS, aux=None, need_dx=True, bias_grad=True, M=None, N=None, xk=None, m_dev=None,
                    rule_M=None):
        """dW += dy^T x ; db += colsum(dy) ; returns dx = epi(dy @ W).  m_dev: device word with the real row count when
        dy / x hold a capacity of rows (the surplus rows must not enter the reduction over rows)."""
        M = dy.shape[0] if M is None else M
        N = lin.N if N is None else N
        self._wgrad(dy, x, lin.gw, M, N, lin.K if xk is None else xk,
                    dbias=lin.gb if (bias_grad and lin.gb is not None) else None, m_dev=m_dev, sole=lin is not self.lin.get("dec"),
                    rule_M=rule_M)
        if not need_dx:
            return None
        dx = torch.empty((M, lin.K), dtype=BF16, device=dy.device)
        kdim = lin.wt.shape[1]
        sk = self._splitk(M, lin.K, kdim)
        if sk is not None:
            L.gemm_nt(dy, lin.wt, dx, bias=None, epilogue=epi, aux=aux, M=M, N=lin.K, K=kdim, tile=sk[0], splitk=sk[1], splitk_ws=sk[2])
        else:
            L.gemm_nt(dy, lin.wt, dx, bias=None, epilogue=epi, aux=aux, M=M, N=lin.K, K=kdim, tile=self._tile(M, lin.K, kdim))
        return dx

    def _decoder_dx(self, dlog, dec, n, V):
        """dhn[n, H] = dlog[n, V] @ E[V, H] for FEW decoded rows (the per-GPU share of a split batch: ~630 rows at 30
        sequences).  As an NT GEMM this is 10 x 6 tiles of 64 x 128, each with a 477-step reduction over the vocabulary:
        60 workgroups on 256 CUs, 348 us -- 3.5 % of the 30-sequence step for 29 GFLOP.  The reduction axis is the long
        one, so it runs on the weight-gradient kernel instead (dW[N, K] += dY[M, N]^T X[M, K] with M = vocabulary,
        dY = dlog^T, X = the bf16 embedding table itself): the vocabulary is cut into S chunks, chunk s is ONE problem of a
        grouped launch with its own zeroed fp32 slab [n, H] (9 tiles of 256 x 256 per chunk, S ~ 27: one round of the chip,
        every tile reduced by one workgroup and written once), and the slabs are added in chunk order and rounded to bf16 by
        one small kernel -- the result does not depend on which workgroup finishes first (atomics into one buffer did:
        rounded to bf16 that showed up as 4e-3 of the gradient scale between two schedules of the same step).
        Costs a bf16 transpose of dlog (38 MB), the slabs (S x 2 MB) and the reduction."""
        H = dec.K
        ldT = _rup(n, 64)
        dlogT = torch.empty((V, ldT), dtype=BF16, device=dlog.device)
        L.transpose_bf16(dlog, dlogT, n, V)
        tiles = ((ldT + 255) // 256) * ((H + 255) // 256)
        S = max(1, min(48, 256 // tiles, V // 1024))
        chunk = _rup((V + S - 1) // S, 64)
        S = max(1, V // chunk)                                 # the last chunk takes the remainder (< 2 chunks long)
        slabs = torch.zeros((S, ldT, H), dtype=F32, device=dlog.device)
        ends = [(s + 1) * chunk for s in range(S - 1)] + [V]
        L.gemm_tn_grouped([(dlogT[e0:e1], dec.w[e0:e1], slabs[s], e1 - e0, ldT, H, None)
                           for s, (e0, e1) in enumerate(zip([0] + ends[:-1], ends))], shared=0)
        dhn = torch.empty((ldT, H), dtype=BF16, device=dlog.device)
        L.sum_slabs_bf16(slabs, dhn, ldT * H)
        return dhn[:n]

    def _layernorm(self, x, key, save, drop=L.NO_DROP, want32=True, lazy=False):
        """x: fp32 pre-LayerNorm sum -> (y32 residual stream | None, y16 GEMM operand, mean, rstd).
        lazy=True: the fp32 output is NOT written; a `_LazyLN` stands in for it and the next residual epilogue
        evaluates LayerNorm(x) from (x, mean, rstd, gamma, beta) itself (4 of the 10 bytes per element this
        HBM-bound kernel moved)."""
        gmm, bta, _, _ = self.ln[key]
        M, H = x.shape
        lazy = lazy and self.lazy_ln and drop[1] == 0
        y32 = torch.empty((M, H), dtype=F32, device=x.device) if (want32 and not lazy) else None
        y16 = torch.empty((M, H), dtype=BF16, device=x.device)
        keep = save or lazy
        mean = torch.empty(M, dtype=F32, device=x.device) if keep else None
        rstd = torch.empty(M, dtype=F32, device=x.device) if keep else None
        L.layernorm_fwd(x, gmm, bta, y32, y16, mean, rstd, M, H, drop=drop)
        if lazy:
            y32 = _LazyLN(x, mean, rstd, gmm, bta)
        return y32, y16, mean, rstd

    def _dense32(self, r):
        """fp32 tensor of a residual-stream value (materialises a lazy LayerNorm output)."""
        if not isinstance(r, _LazyLN):
            return r
        M, H = r.x.shape
        y32 = torch.empty((M, H), dtype=F32, device=r.x.device)
        scratch = torch.empty((M, H), dtype=BF16, device=r.x.device)
        L.layernorm_fwd(r.x, r.gamma, r.beta, y32, scratch, None, None, M, H)
        return y32

    # ------------------------------------------------------------------------------------------
    # image-side stream
    # ------------------------------------------------------------------------------------------
    def _dual(self):
        return self.dual_stream and self.arena.flat.is_cuda

    @staticmethod
    def _touch(obj, stream):
        """Tell the caching allocator that `obj` (allocated on another stream) is read on `stream`."""
        if obj is None:
            return
        if isinstance(obj, _LazyLN):
            for t in (obj.x, obj.mean, obj.rstd):
                t.record_stream(stream)
        elif torch.is_tensor(obj) and obj.is_cuda:
            obj.record_stream(stream)

    def _side_stream(self):
        if self._vside is None:
            self._vside = torch.cuda.Stream(device=self.arena.flat.device)
        return self._vside

    @contextmanager
    def _img(self):
        """Launches inside the block go to the image-side stream, in that stream's order (no waits: use
        `_to_img` / `_to_txt` where the two streams exchange data).  No-op when the dual-stream schedule is off."""
        if not self._dual():
            # one stream: the same schedule serialised -- the block's launches still COUNT as image-side ones (their own
            # weight-gradient queue, i.e. the same grouped launches as the two-stream step, and the image side's tile rule),
            # so that `dual_stream = False` measures the production kernels with the chip to themselves
            was, self._on_side = self._on_side, True
            try:
                yield
            finally:
                self._on_side = was
            return
        side = self._side_stream()
        was, self._on_side = self._on_side, True
        main = self._text_stream
        if was or main is None or L.scoped_stream() is not self._text_scope:   # nested, outside an engine entry, or on a third stream
            try:
                with torch.cuda.stream(side), L.stream_scope(side):
                    yield
            finally:
                self._on_side = was
            return
        # hot path (~110 blocks per step): torch.cuda.stream() costs ~15 us per entry (device-index lookups and a
        # current_stream() query); the text stream of this engine entry is known, so switch and switch back directly
        torch.cuda.set_stream(side)
        try:
            with L.stream_scope(side):
                yield
        finally:
            torch.cuda.set_stream(main)
            self._on_side = was

    @contextmanager
    def _img_if(self, flag):
        if flag:
            with self._img():
                yield
        else:
            yield

    def _to_img(self, *reads):
        """Everything enqueued on the main (text) stream so far happens before whatever the image-side stream is
        given next; `reads` are main-stream tensors the image side is about to use."""
        if not self._dual():
            return
        side = self._side_stream()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        side.wait_event(ev)
        for t in reads:
            self._touch(t, side)

    def _to_txt(self, *reads):
        """The mirror image: the main stream waits for what the image-side stream has been given so far."""
        if not self._dual() or self._vside is None:
            return
        main = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(self._vside)
        main.wait_event(ev)
        for t in reads:
            self._touch(t, main)

    def _layernorm_bwd(self, dy, x, mean, rstd, key, dbias=None, drop=L.NO_DROP, out_drop=L.NO_DROP, defer=True, m_dev=None,
                       drop_rows=None):
        """Row kernel now; the column sums (dgamma, dbeta, dbias) of all the calls of a block are reduced by one grouped
        launch at the end of the block (`_flush_wgrad`), where nothing waits for them.  defer=False: reduce right away."""
        gmm, _, gg, gb = self.ln[key]
        M, H = x.shape
        dx = torch.empty((M, H), dtype=BF16, device=x.device)
        dxd = torch.empty((M, H), dtype=BF16, device=x.device) if drop[1] != 0 else None
        if not defer:
            scratch = (self.part_side if self._on_side else self.part)[H]
            L.layernorm_bwd(dy, x, mean, rstd, gmm, dx, dxd, gg, gb, dbias, scratch, M, H, drop=drop, out_drop=out_drop,
                            drop_rows=drop_rows)
            return dx, (dxd if dxd is not None else dx)
        part = torch.empty(self.part[H].numel(), dtype=F32, device=x.device)      # private until the grouped reduction
        blocks = L.layernorm_bwd_partials(dy, x, mean, rstd, gmm, dx, dxd, part, M, H, drop=drop, out_drop=out_drop, m_dev=m_dev,
                                          drop_rows=drop_rows)
        self._colsum(part, blocks, H, [gg, gb, dbias])
        return dx, (dxd if dxd is not None else dx)

    # ------------------------------------------------------------------------------------------
    # blocks
    # ------------------------------------------------------------------------------------------
    # What a compute mode overrides -- these hooks, `_post_attn`, `_transform_head`, the two embeddings (`_embed_image`,
    # `_embed_text`) and the hooks of the heads' backward (listed above `_transform_head_bwd`); the blocks below and the step
    # around them (`_forward`, `_backward`), their stream brackets, dropout sites and tape entries are written once, against
    # them:
    #   _proj(x, lin)            the fused QKV projection of a block input (x: the GEMM operand of the residual stream)
    #   _attn(...)               -> (ctx, ctx_op, lse): ctx is what the attention backward reads as `out`, ctx_op the operand
    #                            handed to `_post_attn`
    #   _qkv_grad(qkv)           the gradient buffer of a projection output
    #   _attn_bwd(...)           the attention backward into column slices of `_qkv_grad` buffers
    #   _proj_bwd(dqkv, x, lin, add, m_dev)   weight / bias gradients of the projection; returns dx = dqkv @ W + add
    def _proj(self, x, lin):
        return self._linear(x, lin)

    def _attn(self, q, k, v, mask, B, H, Tq, Tk, D, drop, save, qvar=None, kvar=None, tag=None):
        out = torch.empty((q.shape[0], H * D), dtype=BF16, device=q.device)
        lse = torch.empty((B, H, Tq), dtype=F32, device=q.device) if save else None
        words, mq, mb = mask
        L.attn_fwd(q, k, v, out, lse, words, B, H, Tq, Tk, D, 1.0 / math.sqrt(D), mq, mb, drop, qvar=qvar, kvar=kvar)
        if self.attn_sink is not None:          # output_all_attention_masks: the probabilities as tensors (diagnostic, padded layout)
            if qvar is not None or kvar is not None:
                raise RuntimeError("attention probabilities are collected on the padded schedule only")
            probs = torch.empty((B, H, Tq, Tk), dtype=F32, device=q.device)
            L.attn_probs(q, k, probs, words, B, H, Tq, Tk, D, 1.0 / math.sqrt(D), mq, mb, drop)
            self.attn_sink[tag] = probs
        return out, out, lse

    # Inference-only hooks of the shared-context pass (unimm_amd/scoring.py), which launches several attention cores into
    # disjoint row ranges of ONE context buffer (the S rows, then the P rows with the group's rows spliced into their keys)
    # and embeds rows chosen by its own plan:
    #   _ctx_rows(rows, width, device)   an uninitialised context buffer
    #   _attn_rows(q, k, v, ctx, mask, ..., kshared)   one launch into it; no dropout and no lse unless the pass trains
    #                                    (drop / lse given: the bf16 engine's shared-context training step)
    #   _ctx_operand(ctx)                what `_post_attn` takes, once every row is written
    #   _embed_image / _embed_text       the step's embeddings, without dropout and without a backward
    def _ctx_rows(self, rows, width, device):
        return torch.empty((rows, width), dtype=BF16, device=device)

    def _attn_rows(self, q, k, v, ctx, mask, B, H, Tq, Tk, D, qvar=None, kvar=None, kshared=None, drop=L.NO_DROP, lse=None):
        words, mq, mb = mask
        if kshared is not None and lse is not None:          # the spliced launch in its training form
            L.attn_spliced_fwd(q, k, v, ctx, lse, words, B, H, Tq, Tk, D, 1.0 / math.sqrt(D), mq, mb, drop, qvar, kvar, kshared,
                               wide=Tq > 32)
            return
        L.attn_fwd(q, k, v, ctx, lse, words, B, H, Tq, Tk, D, 1.0 / math.sqrt(D), mq, mb, drop, qvar=qvar, kvar=kvar,
                   kshared=kshared)

    def _attn_spliced_bwd(self, q, k, v, ctx, dctx, lse, mask, dq, dk, dv, B, H, Tq, Tk, D, drop, qvar, kvar, kshared, groups):
        """Backward of the spliced `_attn_rows` launch; the groups' shared rows of dk / dv already hold the S x S launch's
        gradient and get the groups' sums on top, in one rounding."""
        words, mq, mb = mask
        L.attn_spliced_bwd(q, k, v, ctx, dctx, lse, dq, dk, dv, words, B, H, Tq, Tk, D, 1.0 / math.sqrt(D), mq, mb, drop, qvar, kvar,
                           kshared, groups, accumulate=True, wide=Tq > 32)

    def _ctx_operand(self, ctx):
        return ctx

    # The two embeddings, for the step and for inference on rows of the caller's choosing (scoring, answer generation call
    # them with L.NO_DROP, save=False) -> (fp32 residual stream, its GEMM operand, bwd | None):
    def _embed_image(self, featd, locd, n, drop, save):
        """Image embedding (models/vilbert_dialog.py:1487-1493) of n regions, featd fp32 [n, F], locd fp32 [n, 5]: one GEMM
        over [feat | loc | 0] with W_cat = [W_feat | W_loc | 0], then LayerNorm."""
        F, Hv, dev = self.cfg.v_feature_size, self.cfg.v_hidden_size, featd.device
        packed = torch.empty((n, self.vemb_k), dtype=BF16, device=dev)
        L.pack_image(featd, locd, packed, n, F, self.vemb_k)
        prev = torch.empty((n, Hv), dtype=F32, device=dev)
        L.gemm_nt(packed, self.vemb_w, prev, bias=self.vemb_b, M=n, N=Hv, K=self.vemb_k)
        xv32, xv, mv, rv = self._layernorm(prev, "emb_v", save, drop=drop)
        if not save:
            return xv32, xv, None
        A, v = self.arena, "bert.v_embeddings."

        def bwd(dxv):
            dbias = A.grad(v + "image_embeddings.bias")
            before = dbias.clone()
            dpre, _ = self._layernorm_bwd(dxv, prev, mv, rv, "emb_v", dbias=dbias, out_drop=drop, defer=False)
            A.grad(v + "image_location_embeddings.bias").add_(dbias - before)
            self._wgrad(dpre, packed, A.grad(v + "image_embeddings.weight"), n, Hv, F, sole=True)
            self._wgrad(dpre, packed[:, F:], A.grad(v + "image_location_embeddings.weight"), n, Hv, 5, sole=True)
        return xv32, xv, bwd

    def _embed_text(self, ids32, pos32, typ32, M, rows, drop, save, m_dev):
        """Text embeddings (:326-356) of M rows; rows (int64 [M]: b * T + t, or None = the first M): the entries of ids32 /
        pos32 / typ32 they embed; m_dev: device word with the valid rows, when M is a capacity."""
        H, dev = self.cfg.hidden_size, ids32.device
        xt = torch.empty((M, H), dtype=BF16, device=dev)
        xt32 = torch.empty((M, H), dtype=F32, device=dev)
        emb = self._embed_text_args(ids32, pos32, typ32)
        L.embed_fwd(*emb, xt32, xt, M, H, self.cfg.type_vocab_size, drop=drop, m_dev=m_dev, rows=rows)
        return xt32, xt, (self._embed_text_bwd(L.embed_bwd, emb, M, rows, drop, m_dev) if save else None)

    def _embed_text_args(self, ids32, pos32, typ32):
        gmm, bta, _, _ = self.ln["emb_t"]
        return (ids32, pos32, typ32, self.tab["word"], self.tab["pos"], self.tab["type"], self.tab["ext"], gmm, bta)

    def _embed_text_bwd(self, kernel, emb, M, rows, drop, m_dev):
        """kernel: L.embed_bwd (bf16 gradient rows) or L.embed_bwd_f32"""
        A, e, H = self.arena, "bert.embeddings.", self.cfg.hidden_size
        _, _, ggm, gbt = self.ln["emb_t"]

        def bwd(dxt):
            kernel(*emb, dxt, A.grad(e + "word_embeddings.weight"), A.grad(e + "position_embeddings.weight"),
                   A.grad(e + "token_type_embeddings.weight"), A.grad(e + "token_type_embeddings_extension.weight"), ggm, gbt,
                   self.part[H], M, H, self.cfg.type_vocab_size, drop=drop, m_dev=m_dev, rows=rows)
        return bwd

    def _embed_text_bwd_ordered(self, ids32, pos32, typ32, M, rows, drop):
        """`_embed_text_bwd` without floating-point atomics (the shared-context training step, bf16): the rows' gradients are
        stored, then added into the word / position / extension-type tables run by run of a stable sort of their table indices
        -- a fixed order of addends, one writer per table row.  The tied decoder's weight gradient is joined first: it adds
        into the same word rows."""
        A, e, H, tv = self.arena, "bert.embeddings.", self.cfg.hidden_size, self.cfg.type_vocab_size
        emb = self._embed_text_args(ids32, pos32, typ32)
        _, _, ggm, gbt = self.ln["emb_t"]
        src = rows if rows is not None else torch.arange(M, device=ids32.device)
        tt = typ32[src]
        lists = []
        for key, name in ((ids32[src], "word_embeddings"), (pos32[src], "position_embeddings"),
                          (torch.where(tt >= tv, tt - tv, torch.full_like(tt, -1)), "token_type_embeddings_extension")):
            ks, order = torch.sort(key.to(torch.int32), stable=True)
            lists.append((ks.contiguous(), order.to(torch.int32), name))

        def bwd(dxt):
            drow = torch.empty((M, H), dtype=F32, device=dxt.device)
            L.embed_bwd_rows(*emb, dxt, drow, A.grad(e + "token_type_embeddings.weight"), ggm, gbt, self.part[H], M, H, tv,
                             drop=drop, rows=rows)
            self._join_wgrad()
            for ks, order, name in lists:
                L.rows_scatter_sum_f32(drow, ks, order, A.grad(e + name + ".weight"))
        return bwd

    def _qkv_grad(self, qkv):
        return torch.empty_like(qkv)

    def _attn_bwd(self, q, k, v, ctx, dctx, lse, mask, dq, dk, dv, N, B, H, Tq, Tk, D, drop, qvar=None, kvar=None):
        """dq / dk / dv: column slices of `_qkv_grad` buffers (N: their projection width, not needed here)."""
        delta = torch.empty_like(lse)
        words, mq, mb = mask
        L.attn_bwd(q, k, v, ctx, dctx, lse, delta, dq, dk, dv, words, B, H, Tq, Tk, D, 1.0 / math.sqrt(D), mq, mb, drop,
                   qvar=qvar, kvar=kvar)

    def _proj_bwd(self, dqkv, x, lin, add, m_dev=None):
        return self._linear_bwd(dqkv, x, lin, L.EPI_ADD, aux=add, m_dev=m_dev)

    def _post_attn(self, ctx, res32, proj, ff1, ff2, ln_mid, ln_out, d_proj, d_ffn, save, m_dev=None, rows=None):
        """What follows the attention in every encoder block: BertSelfOutput or one side of BertBiOutput
        (models/vilbert_dialog.py:744-754), then BertIntermediate, then BertOutput.
        ctx: the attention context; res32: the fp32 residual stream entering the block (possibly a `_LazyLN`); proj, ff1,
        ff2: the three linears; ln_mid, ln_out: keys of `self.ln`; d_proj, d_ffn: the dropout triples of the two residual
        joins; m_dev: device word with the valid rows, when the row dimension is a capacity.
        rows (int32, one per row of ctx): ctx holds a SUBSET of the block's rows, row m being row rows[m] of res32's stream:
        the residual is read there and both joins draw that row's dropout mask, so every row comes out as the block over all
        rows computes it; bwd then maps the subset's dy to the subset's (dctx, dres).
        -> (y32, y, bwd): the fp32 residual stream leaving the block and its bf16 copy; bwd (None unless save) maps dy to
        (dctx, dres), dres being the gradient w.r.t. the first pre-LayerNorm sum: the caller adds it in the epilogue of
        its QKV input-gradient GEMM."""
        pre1 = self._linear(ctx, proj, L.EPI_BIAS_DROP_RESID, aux=res32, drop=d_proj, out_f32=True, drop_rows=rows, aux_rows=rows)
        x1_32, x1, m1, r1 = self._layernorm(pre1, ln_mid, save, lazy=True)
        # training keeps GELU'(u) (not u): the backward epilogue is then a plain multiply
        h, u = self._linear(x1, ff1, L.EPI_BIAS_GELU_DG, want_u=True) if save else (self._linear(x1, ff1, L.EPI_BIAS_GELU), None)
        pre2 = self._linear(h, ff2, L.EPI_BIAS_DROP_RESID, aux=x1_32, drop=d_ffn, out_f32=True, drop_rows=rows)
        x2_32, x2, m2, r2 = self._layernorm(pre2, ln_out, save, lazy=True)
        if not save:
            return x2_32, x2, None

        rm = self._step_rows if rows is not None else None       # the flush rule keeps counting the step's rows (_wgrad)

        def bwd(dx2):
            dpre2, dpre2d = self._layernorm_bwd(dx2, pre2, m2, r2, ln_out, dbias=ff2.gb, drop=d_ffn, m_dev=m_dev, drop_rows=rows)
            du = self._linear_bwd(dpre2d, h, ff2, L.EPI_MUL, aux=u, bias_grad=False, m_dev=m_dev, rule_M=rm)
            dx1 = self._linear_bwd(du, x1, ff1, L.EPI_ADD, aux=dpre2, m_dev=m_dev, rule_M=rm)
            dpre1, dpre1d = self._layernorm_bwd(dx1, pre1, m1, r1, ln_mid, dbias=proj.gb, drop=d_proj, m_dev=m_dev, drop_rows=rows)
            return self._linear_bwd(dpre1d, ctx, proj, bias_grad=False, m_dev=m_dev, rule_M=rm), dpre1
        return x2_32, x2, bwd

    def _self_block(self, key, x32, x, mask, B, T, heads, pname, p_attn, p_hid, st, var=None, prune=None):
        """BertLayer / BertImageLayer (models/vilbert_dialog.py:385-483, :514-612).
        (x32, x): fp32 residual stream and its copy as a GEMM operand (bf16, or the split operand of the fp32x3 mode).
        prune (`_prune_rows`): the block's output is read on those rows only -- projection and attention run on all rows (every
        query attends every key), everything after them on the listed rows; the block then returns, and its backward takes,
        tensors of prune["Mc"] rows."""
        train, tape = st["train"], st["tape"]
        save = tape is not None
        qkv_l, so, ff1, ff2 = (self.lin[key + s] for s in (".qkv", ".so", ".ff1", ".ff2"))
        Hd = qkv_l.N // 3
        D = Hd // heads
        qkv = self._proj(x, qkv_l)
        q, k, v = qkv[:, :Hd], qkv[:, Hd:2 * Hd], qkv[:, 2 * Hd:]
        d_attn = self._drop(pname + "attn", p_attn, train)
        ctx, ctx_op, lse = self._attn(q, k, v, mask, B, heads, T, T, D, d_attn, save, qvar=var, kvar=var, tag=key)
        d_so = self._drop(pname + "so", p_hid, train)
        d_out = self._drop(pname + "out", p_hid, train)
        md = var[2] if var is not None else None      # device word: valid rows, when the row dimension is a capacity
        if prune is None:
            x2_32, x2, post_bwd = self._post_attn(ctx_op, x32, so, ff1, ff2, key + ".ln1", key + ".ln2", d_so, d_out, save, m_dev=md)
        else:
            # (all Mc rows are gathered: the entries past the device count name a valid row, so no operand row is undefined)
            ctx_c = torch.empty((prune["Mc"], ctx_op.shape[1]), dtype=ctx_op.dtype, device=ctx_op.device)
            L.gather_rows(ctx_op, prune["rows"], ctx_c, prune["Mc"], ctx_op.shape[1])
            x2_32, x2, post_bwd = self._post_attn(ctx_c, x32, so, ff1, ff2, key + ".ln1", key + ".ln2", d_so, d_out, save,
                                                  m_dev=prune["m_dev"], rows=prune["rows"])
        if save:
            def bwd(dx2):
                dctx, dpre1 = post_bwd(dx2)
                if prune is not None:
                    dctx, dpre1 = self._unprune(dctx, prune, x.shape[0]), self._unprune(dpre1, prune, x.shape[0])
                dqkv = self._qkv_grad(qkv)
                self._attn_bwd(q, k, v, ctx, dctx, lse, mask, dqkv[:, :Hd], dqkv[:, Hd:2 * Hd], dqkv[:, 2 * Hd:3 * Hd], 3 * Hd,
                               B, heads, T, T, D, d_attn, qvar=var, kvar=var)
                return self._proj_bwd(dqkv, x, qkv_l, dpre1, m_dev=md)
            tape.append((key, bwd))
        return x2_32, x2

    # The last text layer on the rows the losses read.
    prune_supported = True               # (`_post_attn` takes a row list: the bf16 engine)

    def _prune_rows(self, sched, save, lm_rows, sel, dyn, var, B, T, dev):
        """-> None, or what `_self_block(prune=...)` and the heads need to run the last text layer's row-wise half on the rows
        the training losses read.  Only in a step that saves for backward, decodes the labelled rows, whose caller reads no
        sequence output or attention probabilities, and whose last text-side block is a trained text layer; every other path
        runs as it always did.
        rows: the B first-token rows, then the plan's labelled rows in plan order (Mc = B + sel["n"] of them, a capacity; the
        device word m_dev holds B + the real count; the plan gives the surplus entries a valid row).  A first token that carries
        a label is listed twice and computed twice.  In the backward pass its two gradients -- the MLM head's and the pooler's
        -- meet in the labelled copy (cls_dst: where the pooler's input gradient of each sequence is added), as they meet in
        the one row of the all-rows step: the row's gradient is rounded to bf16 once, in the same order, and everything
        upstream of the layer sees the bits it always saw; the first-token copy then carries a zero gradient."""
        if not (self.prune_last_text and self.prune_supported and save and not self._seq_wanted and self.attn_sink is None):
            return None
        if lm_rows != "labelled" or sel is None or sel["n"] <= 0:
            return None
        text_side = [(k, i) for k, i in sched if k == "t" or (k == "c" and self.cfg.with_coattention)]
        if not text_side or text_side[-1][0] != "t" or text_side[-1][1] < self.cfg.fixed_t_layer:
            return None
        cls_idx = var[0] if var is not None else torch.arange(0, B * T, T, dtype=torch.int32, device=dev)
        n = sel["n"]
        first = torch.arange(B, dtype=torch.int32, device=dev)
        # the labelled copy of each first token, if it has one (entries past the device count are fillers, not labelled rows)
        live = torch.arange(n, dtype=torch.int32, device=dev) < dyn["n_lm"]
        match = (sel["idx"][None, :] == cls_idx[:, None]) & live[None, :]
        cls_dst = torch.where(match.any(1), match.to(torch.int32).argmax(1).to(torch.int32) + B, first)
        return dict(layer=text_side[-1][1], B=B, n=n, Mc=B + n, cls_idx=cls_idx, lm_idx=sel["idx"], n_lm_dev=dyn["n_lm"],
                    rows=torch.cat((cls_idx, sel["idx"])), m_dev=dyn["n_lm"] + B, first=first, cls_dst=cls_dst,
                    lm_dst=torch.arange(B, B + n, dtype=torch.int32, device=dev))

    def _unprune(self, g, prune, M):
        """Gradient rows of the pruned layer (bf16 [Mc, W]) -> all M rows, zero elsewhere.  In a fixed order: the labelled rows
        are written (each names its own row), then the first-token rows are added (zero where the labelled copy took the
        first token's gradient: `_prune_rows`)."""
        B, W = prune["B"], g.shape[1]
        full = torch.zeros((M, W), dtype=g.dtype, device=g.device)
        L.gather_rows(g[B:], prune["lm_idx"], full, prune["n"], W, scatter=True, n_dev=prune["n_lm_dev"])
        L.rows_add_f32(full, prune["cls_idx"], g[:B].float(), B, W)
        return full

    def _conn_block(self, key, i, xv32, xv, xt32, xt, B, R, T, vmask, comask, st, var=None):
        """BertConnectionLayer (models/vilbert_dialog.py:655-783)."""
        cfg = self.cfg
        train, tape = st["train"], st["tape"]
        save = tape is not None
        pn = f"bert.encoder.c_layer.{i}."
        Hb, nh = cfg.bi_hidden_size, cfg.bi_num_attention_heads
        D = Hb // nh
        lq1, lq2, d1, d2 = (self.lin[key + s] for s in (".qkv1", ".qkv2", ".d1", ".d2"))
        vff1, vff2, tff1, tff2 = (self.lin[key + s] for s in (".vff1", ".vff2", ".tff1", ".tff2"))
        # The two halves run on their own streams (`_img()` = image side, otherwise the text side); the only
        # exchanges are the other side's K/V for the two co-attention directions.
        with self._img():
            qkv1 = self._proj(xv, lq1)        # image side  [B*R, 3Hb]
        qkv2 = self._proj(xt, lq2)            # text side   [B*T, 3Hb]
        self._to_txt(qkv1)
        self._to_img(qkv2)
        q1, k1, v1 = qkv1[:, :Hb], qkv1[:, Hb:2 * Hb], qkv1[:, 2 * Hb:]
        q2, k2, v2 = qkv2[:, :Hb], qkv2[:, Hb:2 * Hb], qkv2[:, 2 * Hb:]
        da1 = self._drop(pn + "attn1", cfg.v_attention_probs_dropout_prob, train)
        da2 = self._drop(pn + "attn2", cfg.attention_probs_dropout_prob, train)
        db1 = self._drop(pn + "bo1", cfg.v_hidden_dropout_prob, train)
        db2 = self._drop(pn + "bo2", cfg.hidden_dropout_prob, train)
        dvo = self._drop(pn + "vout", cfg.v_hidden_dropout_prob, train)
        dto = self._drop(pn + "tout", cfg.hidden_dropout_prob, train)
        with self._img():
            ctx_v, ctx_v_op, lse_v = self._attn(q1, k2, v2, comask, B, nh, R, T, D, da2, save, kvar=var, tag=key + "/2")    # regions attend text (:701-721)
            ov32, ov, bwd_v = self._post_attn(ctx_v_op, xv32, d1, vff1, vff2, key + ".lnb1", key + ".lnv", db1, dvo, save)   # BertBiOutput (:744-754, call order :775)
        md = var[2] if var is not None else None      # device word: valid text rows (capacity-sized text tensors)
        ctx_t, ctx_t_op, lse_t = self._attn(q2, k1, v1, vmask, B, nh, T, R, D, da1, save, qvar=var, tag=key + "/1")     # text attends regions (:681-698)
        ot32, ot, bwd_t = self._post_attn(ctx_t_op, xt32, d2, tff1, tff2, key + ".lnb2", key + ".lnt", db2, dto, save, m_dev=md)
        if save:
            def bwd(dov, dot):
                # gradient buffers of the two projections: each is written by BOTH attention backward kernels (every
                # slice exactly once), i.e. from both streams -> allocate first and let each stream see the other's
                with self._img():
                    dqkv1 = self._qkv_grad(qkv1)
                dqkv2 = self._qkv_grad(qkv2)
                self._to_txt(dqkv1)
                self._to_img(dqkv2)
                with self._img():                                   # image half: FFN, bi-output
                    dctx_v, dprev = bwd_v(dov)
                    self._attn_bwd(q1, k2, v2, ctx_v, dctx_v, lse_v, comask, dqkv1[:, :Hb], dqkv2[:, Hb:2 * Hb], dqkv2[:, 2 * Hb:3 * Hb],
                                   3 * Hb, B, nh, R, T, D, da2, kvar=var)
                dctx_t, dpret = bwd_t(dot)                          # text half: FFN, bi-output
                self._attn_bwd(q2, k1, v1, ctx_t, dctx_t, lse_t, vmask, dqkv2[:, :Hb], dqkv1[:, Hb:2 * Hb], dqkv1[:, 2 * Hb:3 * Hb],
                               3 * Hb, B, nh, T, R, D, da1, qvar=var)
                self._to_img()                                      # dK1/dV1 written by the text side
                self._to_txt()                                      # dK2/dV2 written by the image side
                with self._img():
                    dxv = self._proj_bwd(dqkv1, xv, lq1, dprev)
                dxt = self._proj_bwd(dqkv2, xt, lq2, dpret, m_dev=md)
                return dxv, dxt
            tape.append((key, bwd))
        return ov32, ov, ot32, ot

    # ------------------------------------------------------------------------------------------
    # inputs
    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _i32(x, device):
        return x.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()

    def stage_host_inputs(self, inp: dict, pack=None):
        """CPU tensors among the step's inputs -> device tensors through the engine's pinned staging ring and copy stream
        (inputs.HostStager; dense masks arrive bit-packed), in place.  Called by the model's forward entry points, so that the
        reference's calling convention -- host tensors handed to forward(), train.py:113-161 -- runs at the speed of resident
        inputs.  `host_staging = False` restores the plain `.to(device)` path."""
        if not self.host_staging or not self.arena.flat.is_cuda:
            return False
        if not any(torch.is_tensor(inp.get(k)) and not inp[k].is_cuda for k in _STAGED_KEYS):
            return False
        if self._stager is None:
            self._stager = HostStager(self.arena.flat.device)
        staged = self._stager.stage(inp, _STAGED_KEYS, pack=pack)
        if staged and self._dual():
            side = self._side_stream()
            # (the co-attention mask: the regions attend the text on the image stream, forward and backward)
            for k in ("image_feat", "image_loc", "image_attention_mask", "image_target", "image_label", "co_attention_mask"):
                v = inp.get(k)
                self._touch(v.words if isinstance(v, PackedMask) else v, side)
        return staged

    def _pack_mask(self, m, device, rows_expected):
        """-> (words, q_stride, b_stride).  m: [B, Tk] (key padding) or [B, Tq, Tk]."""
        if isinstance(m, PackedMask):              # packed on the host side of the copy (inputs.HostStager)
            words = m.words
            nw = words.shape[-1]
            return (words, 0, nw) if m.dim() == 2 else (words, nw, m.shape[1] * nw)
        if m.dtype not in (torch.bool, torch.uint8, torch.int32, torch.int64, torch.float32):
            m = m.float()
        if not m.is_cuda and m.dtype == torch.int64:
            m = m.to(torch.uint8)          # 8x less PCIe traffic for the reference's int64 masks
        m = m.to(device, non_blocking=True)
        words = L.mask_pack(m)
        nw = words.shape[-1]
        self._dev_masks.append(m)
        if m.dim() == 2:
            return (words, 0, nw)
        return (words, nw, m.shape[1] * nw)

    # Unpadded schedule: a text row is INERT when no valid row ever attends it (its column of the text mask and of
    # the co-attention mask is empty), it attends nothing, carries no label / weight and is not the pooled first
    # token: whatever it computes never reaches a loss or a valid row, and its gradient is exactly zero (the
    # reference still spends ~45 % of its token FLOPs there: rows past each dialog's length,
    # models/vilbert_dialog.py:1418 / utils/data_utils.py:207).  The engine runs the text stream on rows
    # [0, len_b) of every sequence only; len_b comes from `unimm_plan_lengths` (see `_forward`).

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    def _on_text_stream(self, fn, *args):
        """Run one engine entry on the text stream.  Normally that is the caller's current stream.  With
        `text_priority` (and two streams) it is an internal HIGH-priority stream bracketed by waits in both
        directions, so that the text kernels - the critical path - are placed before the image side's."""
        if not self.arena.flat.is_cuda:
            return fn(*args)
        caller = torch.cuda.current_stream()
        if not (self.text_priority and self._dual()):
            self._text_stream = caller
            try:
                with L.stream_scope(caller) as sc:
                    self._text_scope = sc.ptr
                    return fn(*args)
            finally:
                self._text_stream = self._text_scope = None
        if self._tstream is None:
            self._tstream = torch.cuda.Stream(device=self.arena.flat.device, priority=-1)
        hp = self._tstream
        hp.wait_stream(caller)
        self._text_stream = hp
        try:
            with torch.cuda.stream(hp), L.stream_scope(hp) as sc:
                self._text_scope = sc.ptr
                return fn(*args)
        finally:
            self._text_stream = self._text_scope = None
            caller.wait_stream(hp)

    def enable_graphs(self, on=True, **kw):
        """Run the training step as two replayed hipGraphs per row-count bucket (unimm_amd/graphs.py) instead of ~650
        Python -> C launches: what the small per-GPU batches of the 8-GPU split need (host-bound otherwise)."""
        from .graphs import StepGraphs
        self.graphs = StepGraphs(self, **kw) if on else None
        return self.graphs

    def count_rows(self, inp: dict, lm_rows="labelled"):
        """The header of the step plan as host values, computed ahead of the step: what `_forward` reads at its one host
        sync.  Same kernels on the same inputs (masks bit-packed, unimm_plan_lengths)."""
        dev = self.arena.device
        ids, feat = inp["input_ids"], inp["image_feat"]
        B, T = ids.shape
        R = feat.shape[1]
        am, im, cm = inp.get("attention_mask"), inp.get("image_attention_mask"), inp.get("co_attention_mask")
        if am is None or isinstance(am, DialogMaskSpec) or cm is None:
            raise ValueError("count_rows needs dense attention_mask / co_attention_mask tensors")
        self._dev_masks = []
        tmask = self._pack_mask(am, dev, T)
        comask = self._pack_mask(cm, dev, R)
        self._dev_masks = []
        return self._plan_header(inp, B, T, R, tmask, comask, dev)[0].tolist()

    def _plan_header(self, inp, B, T, R, tmask, comask, dev, need=True):
        """Conversions of the inputs the plan reads + unimm_plan_lengths -> (header | None, lab32, w32, nw_dev, il32).  Without
        `need` the header is computed only when the NSP class weights live on the device or regions are to be counted."""
        labels, weights = inp.get("masked_lm_labels"), inp.get("lm_weight")
        lab32 = self._i32(labels.reshape(B, T), dev) if labels is not None else None
        w32 = self._i32(weights.reshape(B, T), dev) if (weights is not None and labels is not None) else None
        nw_in = inp.get("nsp_weight")
        nw_dev = nw_in.reshape(-1)[:2].to(F32).contiguous() if (torch.is_tensor(nw_in) and nw_in.is_cuda) else None
        il = inp.get("image_label")
        il32 = self._i32(il.reshape(B, R), dev) if (il is not None and inp.get("image_target") is not None) else None
        header = None
        if need or nw_dev is not None or il32 is not None:
            header = L.plan_lengths(tmask, comask, R, lab32, w32, nw_dev, B, T, image_label=il32)
        return header, lab32, w32, nw_dev, il32

    def forward(self, inp: dict, train: bool, save: bool, lm_rows: str, want_pred_v: bool, want_seq: bool = True):
        """want_seq=False: the caller reads neither out["seq_out_t"] nor out["seq32_t"]; a training step may then run its last
        text layer on the rows the losses read (`_prune_rows`) and return those rows only (out["pruned"])."""
        self._seq_wanted = want_seq
        self._reference_rows(inp)
        try:
            return self._on_text_stream(self._forward, inp, train, save, lm_rows, want_pred_v)
        finally:
            self._seq_wanted = True

    def forward_with_attention(self, inp, train, lm_rows, want_pred_v):
        """Inference forward that also returns the attention probabilities of every layer as the reference's encoder
        collects them under output_all_attention_masks (models/vilbert_dialog.py:834-937): (text layers, image layers,
        connection layers as (text-attends-regions, regions-attend-text)), each fp32 [B, heads, Tq, Tk].  Runs the padded,
        one-stream schedule (the probabilities of padding rows are part of what the reference returns)."""
        was = (self.unpad, self.dual_stream, self.attn_sink)
        self.unpad, self.dual_stream, self.attn_sink = False, False, {}
        try:
            out = self.forward(inp, train=train, save=False, lm_rows=lm_rows, want_pred_v=want_pred_v)
            sink = self.attn_sink
        finally:
            self.unpad, self.dual_stream, self.attn_sink = was

        def order(prefix):
            ks = [k for k in sink if k.startswith(prefix) and "/" not in k]
            return sorted(ks, key=lambda k: int("".join(ch for ch in k if ch.isdigit())))
        att_t = [sink[k] for k in order("t")]
        att_v = [sink[k] for k in order("v")]
        cs = sorted({k.split("/")[0] for k in sink if "/" in k}, key=lambda k: int("".join(ch for ch in k if ch.isdigit())))
        att_c = [(sink[k + "/1"], sink[k + "/2"]) for k in cs]
        return out, (att_t, att_v, att_c)

    def backward(self, out, g_lm, g_img, g_nsp, g_nsp_scores=None):
        return self._on_text_stream(self._backward, out, g_lm, g_img, g_nsp, g_nsp_scores)

    def forward_backward_shared(self, inp: dict, groups, g_lm, train: bool):
        """The LM term's forward and backward over sequences that share their dialog context and image group by group
        (unimm_amd/scoring.py, `train_shared`) -> the LM loss, fp32 [1] (NaN, and nothing added to the gradients, when a
        sequence's context does not match its group's).  g_lm None: the forward and the loss alone."""
        from .scoring import train_shared
        self._reference_rows(inp, groups)
        return self._on_text_stream(train_shared, self, inp, groups, g_lm, train)

    # (lm_weight stays: given weights decide which rows the head decodes -- weight != 0 instead of label != -1 -- and the
    # reference must decode the step's rows; the objectives that refuse lm_weight never carry one)
    _REF_DROPS = (LO.KEY, "image_target", "image_label", "next_sentence_label", "nsp_weight", "_plan_header")

    def _reference_rows(self, inp, groups=None):
        """The step's objective reads a frozen reference model (`objective.reference`, unimm_amd/lm_objective.py): the reference's
        engine runs an inference forward on the step's own inputs -- eval mode, nothing saved, the labelled rows only, on the
        schedule of the step (`groups`: the shared-context pass) -- and leaves its fp32 logits rows in `objective.ref`:
        the same positions in the same order as the rows this engine is about to decode.  Queued ahead of the policy's forward
        on the caller's stream.  The reference's parameters, gradients, dropout counters and training flag are not touched."""
        objective = inp.get(LO.KEY)
        if objective is None or objective.reference is None:
            return
        eng = objective.reference._engine
        eng.ensure(self.arena.device)
        rinp = {k: v for k, v in inp.items() if k not in self._REF_DROPS}
        was = eng.lm_bucket
        eng.lm_bucket = self.lm_bucket         # the same row capacity as the policy's launch (the counts are the step's own)
        try:
            with torch.no_grad():
                if groups is None:
                    lm = eng.forward(rinp, train=False, save=False, lm_rows="labelled", want_pred_v=False).get("lm")
                    objective.ref = lm["logits"] if lm is not None else None
                else:
                    from .scoring import _forward_shared
                    objective.ref = eng._on_text_stream(_forward_shared, eng, rinp, groups, False, None, None, True)["logits"]
        finally:
            eng.lm_bucket = was

    def losses(self, out, inp):
        return self._on_text_stream(self._losses, out, inp)

    def _prep_masks(self, inp, B, T, R, dev):
        """Packed attention masks of the step: (text mask, image key mask, co-attention mask), each (words, q stride, b stride)."""
        ids, feat = inp["input_ids"], inp["image_feat"]
        # ---- masks (models/vilbert_dialog.py:1374-1431) ------------------------------------------
        am = inp.get("attention_mask")
        spec = am if isinstance(am, DialogMaskSpec) else None
        if spec is not None:
            if len(spec) != B or int(spec.length.max()) > T:
                raise ValueError(f"DialogMaskSpec for {len(spec)} sequences / max length {int(spec.length.max())} "
                                 f"does not fit input_ids of shape {tuple(ids.shape)}")
            if inp.get("co_attention_mask") is not None:
                raise ValueError("co_attention_mask must be None when attention_mask is a DialogMaskSpec (it is derived)")
            am = torch.ones((B, T), dtype=torch.uint8, device=dev)      # placeholder, never packed
        if am is None:
            am = torch.ones((B, T), dtype=torch.uint8, device=dev)
        if am.dim() not in (2, 3):
            raise ValueError(f"Wrong shape for txt input_ids (shape {tuple(ids.shape)}) or attention_mask (shape {tuple(am.shape)})")
        im = inp.get("image_attention_mask")
        if im is None:
            im = torch.ones((B, R), dtype=torch.uint8, device=dev)
        if im.dim() not in (2, 3):
            raise ValueError(f"Wrong shape for img input_ids (shape {tuple(feat.shape)}) or attention_mask (shape {tuple(im.shape)})")
        self._dev_masks = []
        if spec is not None:
            # masks synthesised on the device from (mode, L, n)
            tw, cw = L.mask_synth(*spec.to_device(dev), T)
            nw = tw.shape[-1]
            tmask, comask = (tw, nw, T * nw), (cw, 0, nw)
            vmask = self._pack_mask(im, dev, R)
        else:
            cm = inp.get("co_attention_mask")
            if cm is None:
                cm = torch.ones((B, R, T), dtype=torch.uint8, device=dev)
            assert cm.dim() == 3
            tmask = self._pack_mask(am, dev, T)
            vmask = self._pack_mask(im, dev, R)
            comask = self._pack_mask(cm, dev, R)
        self._dev_masks = []
        return tmask, vmask, comask

    def _prep_plan(self, inp, B, T, R, tmask, comask, lm_rows, dev):
        """Input conversions + the plan of the step (one device->host copy): valid prefix lengths of the unpadded schedule,
        the rows the MLM head decodes, loss denominators as device words.  Returns a dict."""
        ids = inp["input_ids"]
        # ---- plan of the step: everything the host has to know, in ONE device->host copy ------------------
        # (valid prefix lengths for the unpadded schedule, the number of rows the MLM head decodes, the NSP class
        # weights when they live on the device); row maps and the decoded rows' index lists are then built on the
        # device.  See csrc/rowops.hip: plan_lengths / plan_build.
        tt = inp.get("token_type_ids")                       # (input conversions go in front of the sync as well)
        ids32 = self._i32(ids.reshape(-1), dev)
        typ32 = self._i32(tt.reshape(-1), dev) if tt is not None else torch.zeros(B * T, dtype=torch.int32, device=dev)
        pos = inp.get("position_ids")
        pos32 = self._i32(pos.reshape(-1), dev) if pos is not None else \
            torch.arange(T, dtype=torch.int32, device=dev).repeat(B)
        labels = inp.get("masked_lm_labels")
        want_sel = lm_rows == "labelled" and labels is not None
        header, lab32, w32, nw_dev, il32 = self._plan_header(inp, B, T, R, tmask, comask, dev, need=self.unpad or want_sel)
        plan, sel, n_img = None, None, None
        dyn = None
        if header is not None:
            # the step's one host sync (the graph executor has read the same header in its pre-pass and injects the values:
            # a captured launch sequence cannot synchronise)
            hh = self._inject_header if self._inject_header is not None else header.tolist()
            n_img = sum(hh[2 * B + 2:3 * B + 2]) if il32 is not None else None
            lens_h, n_lm = hh[:B], (sum(hh[B:2 * B]) if want_sel else 0)
            Mv = sum(lens_h)
            # capacities: what the launches are sized for (= the real counts unless the graph executor set buckets)
            Mcap = min(_rup(Mv, self.row_bucket), B * T)
            ncap = _rup(n_lm, self.lm_bucket) if n_lm > 0 else 0
            # (with row capacities -- the graph executor -- the layout must not depend on whether the bucket happens to reach
            #  B * T: packed even then, with the identity as row map, so that every replay of a signature and the eager step of
            #  the same batch number their rows, and therefore draw their dropout masks, alike)
            unpadded = self.unpad and (Mv < B * T or self.row_bucket > 1)
            # the device words of THIS forward (never shared between forwards: a backward reads the counts of its own step
            # even when other forwards -- an eval pass, a second micro-batch -- ran in between); under a graph capture they come
            # from the graph's pool, i.e. they are static per captured entry
            di, df = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(8, dtype=F32, device=dev)
            built = L.plan_build(header, lab32 if want_sel else None, w32 if want_sel else None, B, T, Mcap if unpadded else Mv,
                                 ncap, want_rows=unpadded, dims=(di, df))
            dyn = dict(m=di[0:1], n_lm=di[1:2], n_img=di[2:3], inv_lm=df[0:1], inv_img=df[1:2])
            if unpadded:
                plan = dict(Mv=Mcap, lens_h=lens_h, rows=built["rows"], inv=built["inv"],
                            var=(built["off"], built["lens"], dyn["m"], built["order"] if self.attn_longest_first else None))
            if want_sel:
                sel = dict(n=ncap, pos=built["lm_pos"], idx=built["lm_idx"] if unpadded else built["lm_pos"],
                           label=built["lm_label"], weight=built["lm_weight"])
            if nw_dev is not None:
                import struct
                st_nspw = struct.unpack("<2f", struct.pack("<2i", hh[2 * B], hh[2 * B + 1]))
            else:
                st_nspw = None
        else:
            st_nspw = None
        self.last_plan = plan
        var = plan["var"] if plan is not None else None
        Mt = plan["Mv"] if plan is not None else B * T      # text rows actually computed
        self._step_rows = Mt

        return dict(ids32=ids32, typ32=typ32, pos32=pos32, labels=labels, lab32=lab32, w32=w32, il32=il32, plan=plan, sel=sel,
                    n_img=n_img, dyn=dyn, st_nspw=st_nspw, var=var, Mt=Mt)

    def _batch_dims(self, inp, dev):
        """Checks the step's shapes -> (B, T, R, image_index as int64 [B] on the device | None)."""
        ids = inp["input_ids"]
        B, T = ids.shape
        feat = inp["image_feat"]
        R = feat.shape[1]
        img_idx = inp.get("image_index")
        if img_idx is not None:
            img_idx = img_idx.to(dev, dtype=torch.int64, non_blocking=True).reshape(-1)
            if img_idx.numel() != B:
                raise ValueError("image_index needs one entry per sequence")
        elif feat.shape[0] != B:
            raise ValueError(f"image_feat has {feat.shape[0]} rows for {B} sequences and no image_index was given")
        if T > 256 or R > 256:
            raise ValueError("sequence / region count above 256 is not supported by the attention kernels")
        return B, T, R, img_idx

    def _pooled_heads(self, xt32, xv32, cls_idx_t, cls_idx_v, B, train):
        """Poolers + NSP head (models/vilbert_dialog.py:946-967, 1064-1070) on rows cls_idx_t / cls_idx_v of the two fp32
        residual streams -> dict of what the heads' backward reads; the logits are `nsp_pad[:, :2]`.
        Everything above the encoder's last LayerNorm runs in fp32 from the fp32 residual stream and the fp32 master
        weights (unimm_linear_f32): 0.4 GFLOP, but with bf16 operands ReLU units of the B pooled rows switched with the
        last bit of the forward and the pooler gradients were 8-16 % off the reference's (round 2)."""
        dev = xt32.device
        H, Hv = xt32.shape[1], xv32.shape[1]
        cls_t = torch.empty((B, H), dtype=F32, device=dev)         # first-token rows (:949, :964)
        cls_v = torch.empty((B, Hv), dtype=F32, device=dev)
        L.gather_rows(xt32.view(BF16), cls_idx_t, cls_t.view(BF16), B, 2 * H)      # fp32 rows moved as 2 H 16-bit elements
        L.gather_rows(xv32.view(BF16), cls_idx_v, cls_v.view(BF16), B, 2 * Hv)
        pooled_t = self._linear32(cls_t, "tpool", relu=True)
        pooled_v = self._linear32(cls_v, "vpool", relu=True)
        d_fuse = self._drop("fuse", 0.1, train)
        fused = torch.empty_like(pooled_t)
        L.mul_dropout(pooled_t, pooled_v, fused, fused.numel(), d_fuse, fusion_sum=self.cfg.fusion_method == "sum")
        nsp = torch.zeros((B, 4), dtype=F32, device=dev)
        self._linear32(fused, "nsp", out=nsp)
        return dict(pooled_t=pooled_t, pooled_v=pooled_v, fused=fused, d_fuse=d_fuse, nsp_pad=nsp, cls_t=cls_t, cls_v=cls_v,
                    cls_idx_t=cls_idx_t, cls_idx_v=cls_idx_v)

    def _forward(self, inp: dict, train: bool, save: bool, lm_rows: str, want_pred_v: bool):
        """Runs the trunk + heads.  Returns a dict of outputs and (when save) the tape for backward.
        lm_rows: 'labelled' (decode only rows that carry a label / weight), 'all', or 'none'."""
        cfg = self.cfg
        dev = self.arena.device
        self.refresh_weights()
        B, T, R, img_idx = self._batch_dims(inp, dev)
        feat = inp["image_feat"]
        st = dict(train=train, tape=[] if save else None)
        tape = st["tape"]

        tmask, vmask, comask = self._prep_masks(inp, B, T, R, dev)
        # ---- image embedding first: it does not depend on the plan, so the image stream already has work while the
        # host waits for the header below (models/vilbert_dialog.py:360-383)
        F = cfg.v_feature_size
        # masks are packed (and the previous step is behind us): the image side may start; it reads the caller's region
        # features and boxes, which may come from any stream's allocator pool (a prefetcher's copy stream)
        self._to_img(feat, inp["image_loc"])
        with self._img():                     # image embedding: beside the first text layers
            featd = feat.to(dev, dtype=F32, non_blocking=True)
            locd = inp["image_loc"].to(dev, dtype=F32, non_blocking=True)
            if img_idx is not None:             # one entry per image on the wire, expanded on the device (train.py:413-432)
                featd, locd = featd.index_select(0, img_idx), locd.index_select(0, img_idx)
            featd, locd = featd.contiguous().view(B * R, F), locd.contiguous().view(B * R, 5)
            xv32, xv, bwd_embv = self._embed_image(featd, locd, B * R, self._drop("emb_v", cfg.hidden_dropout_prob, train), save)

        pl = self._prep_plan(inp, B, T, R, tmask, comask, lm_rows, dev)
        ids32, typ32, pos32, labels = pl["ids32"], pl["typ32"], pl["pos32"], pl["labels"]
        il32, plan, sel, n_img, dyn, st_nspw, var, Mt = (pl[k] for k in ("il32", "plan", "sel", "n_img", "dyn", "st_nspw", "var", "Mt"))
        # ---- embeddings --------------------------------------------------------------------------
        erows = plan["rows"] if plan is not None else None      # packed row -> padded row (the kernels gather through it)
        emd = plan["var"][2] if plan is not None else None
        xt32, xt, bwd_embt = self._embed_text(ids32, pos32, typ32, Mt, erows, self._drop("emb_t", cfg.hidden_dropout_prob, train),
                                              save, emd)

        # ---- encoder (schedule of models/vilbert_dialog.py:842-929) ------------------------------
        # Two streams: the image stream (embedding, image layers, the image half of every connection layer) and the
        # text stream (= the caller's current stream).  They exchange data only inside the connection layers (the
        # co-attention needs the other side's K/V) and meet again before the heads.  Within a segment the image
        # layers are enqueued first so that both queues are fed; the tape keeps each stream's order for backward.
        sched = PM.encoder_schedule(cfg)
        st_frozen = dict(train=train, tape=None)
        pruned = self._prune_rows(sched, save, lm_rows, sel, dyn, var, B, T, dev)
        pos = 0
        while pos < len(sched):
            seg = []
            while pos < len(sched) and sched[pos][0] != "c":
                seg.append(sched[pos])
                pos += 1
            # fixed_t_layer / fixed_v_layer (models/vilbert_dialog.py:850-869): the first layers of a stream run under no_grad in
            # the reference -- here: nothing of them is saved and no backward step is taped, so no gradient reaches them or the
            # stream's embeddings.  with_coattention = False (:901): the connection layers are skipped.
            for kind, i in seg:
                if kind == "v":
                    fz = i < cfg.fixed_v_layer
                    with self._img():
                        xv32, xv = self._self_block(f"v{i}", xv32, xv, vmask, B, R, cfg.v_num_attention_heads,
                                                    f"bert.encoder.v_layer.{i}.", cfg.v_attention_probs_dropout_prob,
                                                    cfg.v_hidden_dropout_prob, st_frozen if fz else st)
                    if save and not fz:
                        tape[-1] = ("v", tape[-1][0], tape[-1][1])
            for kind, i in seg:
                if kind == "t":
                    fz = i < cfg.fixed_t_layer
                    xt32, xt = self._self_block(f"t{i}", xt32, xt, tmask, B, T, cfg.num_attention_heads, f"bert.encoder.layer.{i}.",
                                                cfg.attention_probs_dropout_prob, cfg.hidden_dropout_prob, st_frozen if fz else st, var=var,
                                                prune=pruned if (pruned is not None and i == pruned["layer"]) else None)
                    if save and not fz:
                        tape[-1] = ("t", tape[-1][0], tape[-1][1])
            if pos < len(sched):
                i = sched[pos][1]
                pos += 1
                if cfg.with_coattention:
                    with self._conn_tag():
                        xv32, xv, xt32, xt = self._conn_block(f"c{i}", i, xv32, xv, xt32, xt, B, R, T, vmask, comask, st, var=var)
                    if save:
                        tape[-1] = ("c", tape[-1][0], tape[-1][1])
        # ---- image head (:1001-1005, :1085-1088; its masked KL :1569-1574 is in _losses): on the image stream, beside the
        # text side's last layers and the MLM head
        img = None
        pred_v_out = None
        if want_pred_v or inp.get("image_target") is not None:
            C = cfg.v_target_size
            if not self.image_head_side:
                self._to_txt(xv)              # the head runs on the main stream: it reads what the image stream's last block wrote
            with self._img_if(self.image_head_side):
                tv, uvh, hvn, mh, rh, pred_v = self._transform_head(xv, self.lin["imgtr"], "imgtr", self.lin["imgdec"],
                                                                    _rup(C, 4), save)
            pred_v_out = pred_v.view(B, R, -1)[:, :, :C]
            img = dict(t1=tv, u=uvh, hn=hvn, mean=mh, rstd=rh, pred=pred_v)
        self._to_txt(xv32, xv, img["pred"] if img is not None else None)                # the heads read both streams
        seq_t, seq_v = xt, xv

        xt32, xv32 = self._dense32(xt32), self._dense32(xv32)      # the final residual stream is an output
        out = dict(seq_out_t=seq_t, seq_out_v=seq_v, seq32_t=xt32, seq32_v=xv32, B=B, T=T, R=R, plan=plan, Mt=Mt,
                   nsp_weight_host=st_nspw, n_img=n_img, img_label32=il32, dyn=dyn, img=img, pruned=pruned)
        # (pruned: the text stream's outputs above hold rows `pruned["rows"]` only: first tokens, then the labelled rows)
        if pred_v_out is not None:
            out["pred_v"] = pred_v_out
        # ---- poolers + NSP (models/vilbert_dialog.py:946-967, 1064-1070) -------------------------
        if pruned is not None:
            cls_idx_t = pruned["first"]
        else:
            cls_idx_t = var[0] if var is not None else torch.arange(0, B * T, T, dtype=torch.int32, device=dev)
        cls_idx_v = torch.arange(0, B * R, R, dtype=torch.int32, device=dev)
        heads = self._pooled_heads(xt32, xv32, cls_idx_t, cls_idx_v, B, train)
        out["nsp"] = heads["nsp_pad"][:, :2]

        # ---- MLM head: transform + tied decoder on the selected rows (:982-986, :1023-1026) -------
        V = cfg.vocab_size
        Vp = _rup(V, 64)
        lm = None
        if lm_rows == "labelled" and labels is not None:
            n = sel["n"]                                          # rows chosen by the plan kernels at the start of forward (a capacity)
            if n > 0:
                W = seq_t.shape[1]                                # the operand's own width: split rows move as 3 H 16-bit elements
                if pruned is not None:
                    xs = seq_t[B:]                                # the last layer ran on these rows: they are in place
                else:
                    xs = torch.empty((n, W), dtype=BF16, device=dev)
                    L.gather_rows(seq_t, sel["idx"], xs, n, W, n_dev=dyn["n_lm"])
                lm = self._lm_head(xs, n, sel["label"], sel["weight"], save, n_dev=dyn["n_lm"],
                                   objective=inp.pop(LO.KEY, LO.LIKELIHOOD), pos=sel["pos"])     # (moved: `inp` keeps nothing of it)
                lm.update(idx=sel["idx"], pos_idx=sel["pos"], n=n, n_dev=dyn["n_lm"], inv_dev=dyn["inv_lm"])
            out["lm"] = lm
        elif lm_rows == "all":
            out["pred_t"] = self.decode_rows(self.padded(out, seq_t), B * T).view(B, T, Vp)[:, :, :V]

        if save:
            out["bwd"] = dict(tape=tape, embt=bwd_embt, embv=bwd_embv, **heads)
        return out

    @staticmethod
    def padded(out, x):
        """[rows computed, H] -> the reference's [B*T, H] layout (rows that were never computed are zero)."""
        if out.get("pruned") is not None:
            raise RuntimeError("this step ran its last text layer on the loss rows only (Engine.forward(want_seq=False)): "
                               "it has no sequence output")
        plan = out.get("plan")
        if plan is None:
            return x
        full = torch.zeros((out["B"] * out["T"], x.shape[1]), dtype=x.dtype, device=x.device)
        if "rows32" not in plan:
            plan["rows32"] = plan["rows"].to(torch.int32)
        src, w = _rows16(x)
        # the row dimension of x is a capacity: only the step's real rows are scattered (device-side count)
        L.gather_rows(src, plan["rows32"], _rows16(full)[0], x.shape[0], w, scatter=True, n_dev=plan["var"][2])
        return full

    def _transform_head(self, x, tr, ln_key, dec, ldo, save, M=None):
        """transform -> GELU -> LayerNorm -> decoder of the MLM and image heads (models/vilbert_dialog.py:982-986, :1001-1005)
        on M rows of the GEMM operand x -> (t, u, hn, mean, rstd, out): the fp32 GELU output, the transform's pre-activation
        (None unless save), the normalised decoder operand, the LayerNorm statistics (None unless save), fp32 out [M, ldo]."""
        if save:
            t, u = self._linear(x, tr, L.EPI_BIAS_GELU, want_u=True, out_f32=True, M=M)
        else:
            t, u = self._linear(x, tr, L.EPI_BIAS_GELU, out_f32=True, M=M), None
        _, hn, mean, rstd = self._layernorm(t, ln_key, save, want32=False)
        return t, u, hn, mean, rstd, self._linear(hn, dec, out_f32=True, ldo=ldo)

    def _lm_head(self, xs, n, lab_sel, w_sel, save, n_dev=None, objective=LO.LIKELIHOOD, pos=None):
        """The MLM head on the n decoded rows xs and the forward row kernels of the step's objective (unimm_amd/lm_objective.py;
        pos: the rows' flat positions) -> the head's state, which carries the objective to `_losses` and `_lm_loss_grad`."""
        V = self.cfg.vocab_size
        objective.stage(pos, xs.device)
        t1, u, hn, mean, rstd, logits = self._transform_head(xs, self.lin["lmtr"], "lmtr", self.lin["dec"], _rup(V, 64), save)
        rowloss, rownll, lse = (torch.empty(n, dtype=F32, device=xs.device) for _ in range(3))
        lm = dict(xs=xs, t1=t1, u=u, hn=hn, mean=mean, rstd=rstd, logits=logits, rowloss=rowloss, rownll=rownll, lse=lse,
                  labels=lab_sel, weights=w_sel, objective=objective)
        objective.forward(self, lm, n, n_dev)
        return lm

    def decode_rows(self, x, n):
        """MLM transform + decoder for n rows of the GEMM operand x, fp32 logits [n, Vpad] (no loss, nothing saved)."""
        return self._transform_head(x, self.lin["lmtr"], "lmtr", self.lin["dec"], _rup(self.cfg.vocab_size, 64), False, M=n)[5]

    # The heads' backward, like the blocks, is written once (`_backward`) against what a compute mode overrides:
    #   grad_dtype               element type of the gradient of the residual streams
    #   _lm_loss_grad / _img_loss_grad   the loss gradient w.r.t. a head's output, as the operand of its decoder's backward
    #   _transform_head_bwd      the mirror of `_transform_head`
    #   _rows_add                fp32 rows added onto rows of a gradient stream (the poolers' input gradients)
    grad_dtype = BF16

    def _gvec(self, g):
        """A loss's incoming gradient as an fp32 [1] device tensor (None: the loss does not take part)."""
        dev = self.arena.device
        return torch.zeros(1, dtype=F32, device=dev) if g is None else g.detach().to(F32).reshape(1).contiguous()

    def _lm_loss_grad(self, lm, g_lm):
        n, V = lm["n"], self.cfg.vocab_size          # n is a capacity: the real count lives on the device (n_dev)
        dlog = torch.empty((n, _rup(V, 64)), dtype=BF16, device=self.arena.device)
        lm["objective"].backward(self, lm, self._gvec(g_lm), dlog)
        return dlog

    def _img_loss_grad(self, img, gimg, rows):
        C = self.cfg.v_target_size
        dpred = torch.empty((rows, self.lin["imgdec"].wt.shape[1]), dtype=BF16, device=self.arena.device)
        if self.cfg.predict_feature:
            L.mse_loss_bwd(img["pred"], img["target"], img["label"], gimg, img["inv"], dpred, rows, C)
        else:
            L.kl_loss_bwd(img["pred"], img["target"], img["label"], img["lse"], gimg, img["inv"], dpred, rows, C,
                          inv_dev=img.get("inv_dev"))
        return dpred

    def _transform_head_bwd(self, dout, hs, x, tr, ln_key, dec, M=None, N=None, m_dev=None):
        """dout: the loss gradient w.r.t. the head's output (M rows, N valid columns); hs: what `_transform_head` returned, by
        name (t1, u, hn, mean, rstd); x: the head's input operand.  Accumulates the head's parameter gradients -> dx."""
        M = dout.shape[0] if M is None else M
        if dec is self.lin["dec"] and M <= self.skinny_dx_rows:      # dE += dlog^T hn ; dbias ; dhn = dlog @ E
            self._linear_bwd(dout, hs["hn"], dec, M=M, N=N, m_dev=m_dev, need_dx=False)
            dhn = self._decoder_dx(dout, dec, M, N)
        else:
            dhn = self._linear_bwd(dout, hs["hn"], dec, M=M, N=N, m_dev=m_dev)
        dt, _ = self._layernorm_bwd(dhn, hs["t1"], hs["mean"], hs["rstd"], ln_key, m_dev=m_dev)
        du = torch.empty_like(dt)
        L.gelu_bwd(dt, hs["u"], du, du.numel())
        return self._linear_bwd(du, x, tr, m_dev=m_dev)

    def _rows_add(self, dst, idx, src, n):
        L.rows_add_f32(dst, idx, src, n, src.shape[1])

    # ------------------------------------------------------------------------------------------
    # losses + backward
    # ------------------------------------------------------------------------------------------
    def _losses(self, out, inp):
        """Three shape-[1] fp32 losses from the forward state (models/vilbert_dialog.py:1559-1621)."""
        cfg = self.cfg
        dev = self.arena.device
        B, R = out["B"], out["R"]
        res = {}
        lm = out.get("lm")
        # (nothing labelled: 0 / 0 in the reference)
        res["lm_loss"] = torch.full((1,), float("nan"), dtype=F32, device=dev) if lm is None else lm["objective"].loss(self, lm)
        # image KL
        img = out["img"]
        C = cfg.v_target_size
        label = inp["image_label"]
        n_img = out["n_img"] if out.get("n_img") is not None else int((label == 1).sum())     # counted by the step plan
        tgt = inp["image_target"].to(dev, dtype=F32, non_blocking=True)
        if inp.get("image_index") is not None and tgt.shape[0] != B:
            tgt = tgt.index_select(0, inp["image_index"].to(dev, dtype=torch.int64).reshape(-1))
        tgt = tgt.contiguous().view(B * R, C)
        lab32 = out["img_label32"].reshape(-1) if out.get("img_label32") is not None else self._i32(label.reshape(-1), dev)
        rl, lse = torch.empty(B * R, dtype=F32, device=dev), torch.empty(B * R, dtype=F32, device=dev)
        img_loss = torch.empty(1, dtype=F32, device=dev)
        if cfg.predict_feature:               # MSE on the labelled regions / max(#selected elements, 1) (:1562-1566)
            L.mse_loss_fwd(img["pred"], tgt, lab32, rl, B * R, C)
            inv_img, inv_img_dev = 1.0 / max(n_img, 1), None
        else:
            L.kl_loss_fwd(img["pred"], tgt, lab32, rl, lse, B * R, C)
            inv_img = 1.0 / n_img if n_img > 0 else float("inf")
            # (the plan kernels counted the regions: the divisor is then read from the device word, not from a launch argument)
            inv_img_dev = out["dyn"]["inv_img"] if (out.get("dyn") is not None and out.get("n_img") is not None) else None
        L.reduce_sum(rl, B * R, img_loss, inv_img, scale_dev=inv_img_dev)
        img.update(target=tgt, label=lab32, lse=lse, inv=inv_img, inv_dev=inv_img_dev)
        res["img_loss"] = img_loss
        # NSP
        nw = inp.get("nsp_weight")
        if nw is None:
            w0, w1 = 1.0, 1.0
        else:
            w = out["nsp_weight_host"] if out.get("nsp_weight_host") is not None else \
                [float(x) for x in nw.reshape(-1, 2)[0].tolist()]          # host tensor: no device round trip
            w0, w1 = 1.0, w[1] / w[0]
        nlab = self._i32(inp["next_sentence_label"].reshape(-1), dev)
        nsp_loss = torch.empty(1, dtype=F32, device=dev)
        L.nsp_loss_fwd(out["bwd"]["nsp_pad"] if "bwd" in out else out["nsp"], nlab, w0, w1, nsp_loss, B)
        out["nsp_state"] = (nlab, w0, w1)
        res["nsp_loss"] = nsp_loss
        return res

    def _backward(self, out, g_lm, g_img, g_nsp, g_nsp_scores=None):
        """Accumulates every parameter gradient into the arena (+=)."""
        cfg = self.cfg
        dev = self.arena.device
        bw = out["bwd"]
        B, R = out["B"], out["R"]
        self.arena.attach_grads()
        self._bwd_fresh = bool(self.arena.fresh)   # gradients known to be zero: sole contributors may write instead of add (_wgrad)
        self._ledger.begin()                       # no gradient bucket reported done in this pass yet (_bucket_done)
        if self._bwd_fresh and self.debug_fresh and bool(self.arena.grad_flat.any()):
            raise RuntimeError("the gradient arena is marked fresh (zeroed since the last backward) but holds non-zero values: "
                               "something wrote into .grad / grad_flat between zero_grad() and backward() without clearing "
                               "`model.engine.arena.fresh` (INTEGRATION.md, 'Gradient arena')")
        self._step_rows = out["Mt"]              # the tile rule follows THIS step's rows (another forward may have run since)

        pruned = out.get("pruned")                # the text stream ends on the loss rows: first tokens, then the labelled rows
        dseq_t = torch.zeros((out["Mt"] if pruned is None else pruned["Mc"], cfg.hidden_size), dtype=self.grad_dtype, device=dev)
        # ---- image head: on the image stream, beside the MLM head's backward -------------------------
        img = out["img"]
        gimg = self._gvec(g_img)
        self._to_img(gimg, img["target"], img["lse"], img["label"])
        with self._img_if(self.image_head_side):
            dpred = self._img_loss_grad(img, gimg, B * R)
            dseq_v = self._transform_head_bwd(dpred, img, out["seq_out_v"], self.lin["imgtr"], "imgtr", self.lin["imgdec"], M=B * R,
                                              N=cfg.v_target_size)
        # ---- MLM head ---------------------------------------------------------------------------
        lm = out.get("lm")
        if lm is not None:
            n, nd = lm["n"], lm.get("n_dev")
            dxs = self._transform_head_bwd(self._lm_loss_grad(lm, g_lm), lm, lm["xs"], self.lin["lmtr"], "lmtr", self.lin["dec"],
                                           M=n, N=cfg.vocab_size, m_dev=nd)
            src, w = _rows16(dxs)
            L.gather_rows(src, lm["idx"] if pruned is None else pruned["lm_dst"], _rows16(dseq_t)[0], n, w, scatter=True, n_dev=nd)
        # ---- NSP + poolers ------------------------------------------------------------------------
        nlab, w0, w1 = out["nsp_state"]
        dnsp = torch.empty((B, 2), dtype=F32, device=dev)
        extra = None                      # gradient arriving through the returned NSP scores (dense fine-tune ranking loss)
        if g_nsp_scores is not None:
            extra = g_nsp_scores.detach().to(device=dev, dtype=F32).reshape(B, 2).contiguous()
        L.nsp_loss_bwd(bw["nsp_pad"], nlab, w0, w1, self._gvec(g_nsp), dnsp, B, extra=extra)
        dfused = self._linear32_bwd(dnsp, bw["fused"], "nsp")
        dpt, dpv = torch.empty_like(dfused), torch.empty_like(dfused)
        L.mul_dropout_bwd(bw["pooled_t"], bw["pooled_v"], dfused, dpt, dpv, dfused.numel(), bw["d_fuse"],
                          fusion_sum=cfg.fusion_method == "sum")
        # pooler input gradients land on the first-token rows
        dcls_t = self._linear32_bwd(dpt, bw["cls_t"], "tpool")
        self._rows_add(dseq_t, bw["cls_idx_t"] if pruned is None else pruned["cls_dst"], dcls_t, B)
        dcls_v = self._linear32_bwd(dpv, bw["cls_v"], "vpool")
        self._to_img(dcls_v)                     # the image pooler's input gradient joins the image head's on the image stream
        with self._img_if(self.image_head_side):
            self._rows_add(dseq_v, bw["cls_idx_v"], dcls_v, B)
        self._bucket_done("heads")
        # ---- encoder blocks in reverse -------------------------------------------------------------
        gt, gv = dseq_t, dseq_v
        entries = list(reversed(bw["tape"]))
        if not self.image_head_side:
            self._to_img(gv)                     # the heads' gradient of the image stream was produced on the main stream
        self._backward_encoder(bw, entries, gt, gv)
        self._to_txt()                                       # everything joined before the caller continues
        self._bucket_done("text_embeddings")
        self.arena.fresh = False                             # the arena holds this pass's gradients now
        self._bwd_fresh = False

    def _backward_encoder(self, bw, entries, gt, gv):
        """The encoder blocks of the tape in reverse (`entries`), then the two embedding backward passes; every block's bucket
        is reported as it completes (`_bucket_done`).  Shared by the bf16 and the fp32x3 engine."""
        pos = 0
        embv_done = False

        def image_tail():
            # The image stream's last work -- the image embedding's backward -- is enqueued as soon as no image or connection
            # layer is left on the tape (the full config: after c0, with text layers 5..0 still to come), and the image side's
            # queued weight gradients are launched with it: under data parallelism the image-side buckets (v0, c0's image half,
            # the image embedding) then travel while the remaining text layers run, instead of after the end of backward behind
            # everything else (bucket_plan.py: the last collective of an 8-rank step shrinks from 392 MB to 181 MB).
            nonlocal embv_done
            if embv_done or any(e[0] in ("c", "v") for e in entries[pos:]):
                return
            embv_done = True
            with self._img():
                if self.cfg.fixed_v_layer == 0:              # (frozen lower image layers: no gradient reaches the image embedding)
                    bw["embv"](gv)
                self._bucket_done("image_embeddings", force_img=True)

        while pos < len(entries):
            image_tail()
            seg = []
            while pos < len(entries) and entries[pos][0] != "c":
                seg.append(entries[pos])
                pos += 1
            for kind, key, fn in seg:                        # image layers of this segment beside its text layers
                if kind == "v":
                    with self._img():
                        gv = fn(gv)
                        self._bucket_done(key)
            for kind, key, fn in seg:
                if kind == "t":
                    gt = fn(gt)
                    self._bucket_done(key)
            if pos < len(entries):
                _, key, fn = entries[pos]
                pos += 1
                with self._conn_tag():
                    gv, gt = fn(gv, gt)                      # exchanges between the streams happen inside
                self._bucket_done(key)
        image_tail()
        if self.cfg.fixed_t_layer == 0:
            bw["embt"](gt)
        # blocks without a backward step (frozen layers, connection layers under with_coattention = False) still own a gradient
        # bucket: report them, so that a data-parallel wrapper sees every bucket once per step (their gradients are zero / None)
        for g, _, _ in self.arena.buckets:
            if g not in self._ledger.reported and g != "text_embeddings":
                self._bucket_done(g)

    def _bucket_done(self, group, force_img=False):
        """A block's backward is enqueued: mark it in the ledger, launch the sides the ledger names and call the data-parallel
        hook with the buckets it hands over.  A block's weight gradients may stay queued for a later grouped launch; its bucket
        is handed over once the launches that cover it are enqueued (`bucket_plan.Ledger.mark`, which the planner drives too)."""
        last = group == "text_embeddings"
        force = last or group == "heads"          # the decoder's gradient has its own row count: a launch of its own
        hook = self.grad_bucket_hook
        sides, ready = self._ledger.mark(group, self.wgrad_group_rounds, self._on_side, force, force_img, hand_over=hook is not None)
        self._flush_wgrad(sides=sides)
        if ready or (last and hook is None):      # before the exchange reads them, or (last bucket) before the caller continues:
            self._join_wgrad()                    # every grouped launch so far joined into this stream ...
            self._to_txt()                        # ... including the ones the image side produced
        for g, more in ready:
            hook(g, more)                         # more: the next bucket follows at once (adjacent slices travel together)
        assert not (last and self._ledger.pending), self._ledger.pending
