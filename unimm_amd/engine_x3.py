"""The fp32-accuracy engine ("fp32x3"): the launch schedule of `unimm_amd.engine.Engine` with fp32 activations,
fp32 gradients and fp32-grade GEMMs, for callers that run the reference WITHOUT autocast
(dense_annotation_finetuning.py:253 calls `forward` in fp32 end to end; north_star gates fp32 results at 1e-3).

gfx950 has no fast fp32 matrix path, so every nn.Linear still runs on the bf16 MFMA GEMM kernels, over SPLIT operands
(include/unimm_hip.h "fp32x3"): x = hi + lo, an activation operand is [hi | lo | hi], a weight operand [hi | hi | lo], and
one GEMM over the three-plane reduction axis gives hi hi + lo hi + hi lo in an fp32 accumulator (~2^-16 relative).  Every
GEMM writes fp32; the kernels of csrc/x3ops.hip turn fp32 results into the next split operand (with the GELU / GELU' /
residual-join that the bf16 path fuses into GEMM epilogues), run LayerNorm / embedding / loss backward on fp32 gradients,
and compute the attention cores in fp32 on the vector ALUs.  Masks, the unpadded schedule, dropout counters, the row-sparse
decoder, the fp32 pooler / NSP heads, the loss kernels and the flat gradient arena are the base engine's.

The encoder blocks, the MLM head and `decode_rows` are the base engine's own code, not a copy: this class overrides the
operand hooks they are written against (`_proj`, `_attn`, `_qkv_grad`, `_attn_bwd`, `_proj_bwd`, `_post_attn`,
`_transform_head`).  So is the step: `_forward`, `_backward` and `_backward_encoder` exist in the base engine only, written
against the embedding hooks (`_embed_image`, `_embed_text`) and the hooks of the heads' backward (`grad_dtype`,
`_lm_loss_grad`, `_img_loss_grad`, `_transform_head_bwd`, `_rows_add`); `_forward` here only refuses the encoder options
this mode does not run.  The base engine's two-stream schedule (image side beside the text side), eager launches or the
graph executor, no lazy LayerNorm: this is the accuracy mode, ~0.3 of the bf16 engine's throughput.  There is no CPU /
eager-PyTorch fallback here either."""
from __future__ import annotations

import math

import torch

from . import lib as L
from .engine import BF16, F32, Engine, _rup


class _Lin3:
    """One (possibly fused) linear of the fp32x3 mode: fp32 master weight view [N, K], its w-type split [N, 3 Kp], the
    transposed w-type split [K, 3 Np] (input-gradient operand), fp32 bias, gradient views."""
    __slots__ = ("w32", "w3", "wt3", "bias", "gw", "gb", "N", "K", "Np", "Kp")

    def __init__(self, w32, bias, gw, gb, device, make_wt=True):
        self.w32, self.bias, self.gw, self.gb = w32, bias, gw, gb
        self.N, self.K = w32.shape
        self.Np, self.Kp = _rup(self.N, 64), _rup(self.K, 64)
        self.w3 = torch.zeros((self.N, 3 * self.Kp), dtype=BF16, device=device)
        self.wt3 = torch.zeros((self.K, 3 * self.Np), dtype=BF16, device=device) if make_wt else None


class EngineX3(Engine):
    compute_dtype = "fp32x3"

    def __init__(self, model, cfg):
        super().__init__(model, cfg)
        self.dual_stream = True           # the base engine's two-stream schedule (image side beside the text side)
        self.lazy_ln = False
        self.splitk = True                # small batches: the long reductions (K = 3 x 768 ... 3 x 3072) as two workgroups per tile
        self.attn_planes = True      # attention kernels write the next GEMM's split operand themselves (matrix kernels; False for
                                     # A/B runs of the vector kernels: fp32 result + a split pass)

    # ------------------------------------------------------------------------------------------
    # weights: split copies instead of the bf16 copies
    # ------------------------------------------------------------------------------------------
    def _mk_lin(self, key, wnames, bnames, device, kpad=None, make_wt=True):
        _, w32, gw = self._fused(wnames)
        _, b32, gb = self._fused(bnames) if bnames else (None, None, None)
        self.lin[key] = _Lin3(w32, b32, gw, gb, device, make_wt)

    def _build_tables(self, device):
        super()._build_tables(device)
        cfg = self.cfg
        self.vemb_w32 = torch.zeros((cfg.v_hidden_size, self.vemb_k), dtype=F32, device=device)   # [W_feat | W_loc | 0]
        self.vemb_w3 = torch.zeros((cfg.v_hidden_size, 3 * self.vemb_k), dtype=BF16, device=device)

    def refresh_weights(self, force=False, cast=True):
        """fp32 arena -> w-type split copies (and their transposes for the input-gradient GEMMs)."""
        A = self.arena
        ver = self._weight_version()
        if not force and ver == self._w_version:
            return
        for lin in self.lin.values():
            L.x3_split(lin.w32, out3=lin.w3, rows=lin.N, cols=lin.K, cp=lin.Kp, wtype=True)
            if lin.wt3 is not None:
                L.x3_split_wt(lin.w32, lin.wt3, lin.N, lin.K, lin.Np)
        cfg = self.cfg
        F = cfg.v_feature_size
        v = "bert.v_embeddings."
        self.vemb_w32[:, :F].copy_(A.view(v + "image_embeddings.weight"))
        self.vemb_w32[:, F:F + 5].copy_(A.view(v + "image_location_embeddings.weight"))
        L.x3_split(self.vemb_w32, out3=self.vemb_w3, wtype=True)
        torch.add(A.view(v + "image_embeddings.bias"), A.view(v + "image_location_embeddings.bias"), out=self.vemb_b)
        self._w_version = ver

    # (enable_graphs is the base engine's: the fp32x3 launch sequence carries the same device-side row counts, loss
    #  denominators and dropout salt word through its kernels, so unimm_amd/graphs.py captures and replays it unchanged --
    #  round 5; configs[3] on 8 GPUs is 12-13 sequences per rank in this arithmetic class, where ~17 ms of host calls per
    #  eager step would otherwise bound the step)

    def _splitk(self, M, N, K):
        """(tile code, splitk, workspace) for a GEMM of the small-batch regime, or None.  Every reduction of this mode is three
        planes long (K = 2304 ... 9216) while a per-rank share of configs[3] has ~1.7k text rows: 162 tiles of 64x128, each a
        36-144 step chain.  Measured at 1,700 rows (profiles/r5*_x3_small_batch_gemm_microbench.txt): N = 768, K = 9216 78.7 us ->
        41.5 us as 128x128 tiles with four workgroups per tile; K = 2304 / 3072 22.3 / 30.2 -> 18.1 / 24.1 us on the 3-slot ring
        of the 64x128 tile (two K steps in flight), no split.  (Four splits: the sum's last bits depend on which split arrives
        last, like the atomically accumulated weight gradients.)"""
        if not self.splitk or self._on_side or self.gemm_tile != 0 or self._step_rows is None or self._step_rows >= self.small_rows:
            return None
        if M != self._step_rows or N > 1024 or K < 2048:
            return None
        t128 = ((M + 127) // 128) * ((N + 127) // 128)
        if K >= 6144 and 2 * t128 <= 512:
            return 1, (4 if 4 * t128 <= 512 else 2), self._splitk_workspace()
        if ((M + 63) // 64) * ((N + 127) // 128) <= 512:
            return 9, 0, None
        return None

    # ------------------------------------------------------------------------------------------
    # helpers
    # ------------------------------------------------------------------------------------------
    def _op3(self, a, op=L.X3_COPY, b=None, want3=True, want32=False, rows=None, cols=None):
        """y = op(a, b) in fp32 -> (split operand [rows, 3 cp] | None, fp32 [rows, cols] | None)"""
        rows = a.shape[0] if rows is None else rows
        cols = a.shape[1] if cols is None else cols
        cp = _rup(cols, 64)
        o3 = torch.empty((rows, 3 * cp), dtype=BF16, device=a.device) if want3 else None
        o32 = torch.empty((rows, cols), dtype=F32, device=a.device) if want32 else None
        L.x3_split(a, out3=o3, out32=o32, op=op, b=b, rows=rows, cols=cols, cp=cp)
        return o3, o32

    def _split(self, a, rows=None, cols=None):
        return self._op3(a, rows=rows, cols=cols)[0]

    def _lin3(self, x3, lin, epi=L.EPI_BIAS, aux=None, drop=None, ldo=None, M=None, bias=True):
        M = x3.shape[0] if M is None else M
        out = torch.empty((M, ldo or lin.N), dtype=F32, device=x3.device)
        sk = self._splitk(M, lin.N, 3 * lin.Kp)
        skw = dict(tile=sk[0], splitk=sk[1], splitk_ws=sk[2]) if sk is not None else {}
        L.gemm_nt(x3, lin.w3, out, bias=lin.bias if bias else None, epilogue=epi, aux=aux, drop=drop, M=M, N=lin.N, K=3 * lin.Kp, **skw)
        return out

    def _wgrad3(self, dy3, x3, gw, M, N, K, Np, Kp, dbias=None, m_dev=None, xcol0=0):
        """dW += dY^T X on split operands: (hi, hi) + (lo, hi) + (hi, lo); the bias gradient = column sums of hi + lo."""
        xh, xl = x3[:, xcol0:xcol0 + K], x3[:, Kp + xcol0:Kp + xcol0 + K]
        self._wgrad(dy3[:, :N], xh, gw, M, N, K, dbias=dbias, m_dev=m_dev)
        self._wgrad(dy3[:, Np:Np + N], xh, gw, M, N, K, dbias=dbias, m_dev=m_dev)
        self._wgrad(dy3[:, :N], xl, gw, M, N, K, dbias=None, m_dev=m_dev)

    def _lin3_bwd(self, dy3, x3, lin, need_dx=True, bias_grad=True, M=None, m_dev=None, add=None):
        """dW += dy^T x ; db += colsum(dy) ; returns dx = dy @ W [+ add] (fp32) or None.  `add` (fp32 [M, K]): the other
        gradient that meets dx at a residual fork, added in the GEMM's residual epilogue instead of a pass of its own."""
        M = dy3.shape[0] if M is None else M
        self._wgrad3(dy3, x3, lin.gw, M, lin.N, lin.K, lin.Np, lin.Kp,
                     dbias=lin.gb if (bias_grad and lin.gb is not None) else None, m_dev=m_dev)
        if not need_dx:
            return None
        dx = torch.empty((M, lin.K), dtype=F32, device=dy3.device)
        sk = self._splitk(M, lin.K, 3 * lin.Np)
        skw = dict(tile=sk[0], splitk=sk[1], splitk_ws=sk[2]) if sk is not None else {}
        if add is None:
            L.gemm_nt(dy3, lin.wt3, dx, bias=None, M=M, N=lin.K, K=3 * lin.Np, **skw)
        else:
            L.gemm_nt(dy3, lin.wt3, dx, bias=None, epilogue=L.EPI_BIAS_DROP_RESID, aux=add, M=M, N=lin.K, K=3 * lin.Np, **skw)
        return dx

    def _ln3(self, x, key, save, drop=L.NO_DROP, want3=True):
        """x: fp32 pre-LayerNorm sum -> (y32, y3 split operand, mean, rstd)"""
        gmm, bta, _, _ = self.ln[key]
        M, H = x.shape
        y32 = torch.empty((M, H), dtype=F32, device=x.device)
        mean = torch.empty(M, dtype=F32, device=x.device) if save else None
        rstd = torch.empty(M, dtype=F32, device=x.device) if save else None
        if not want3:
            L.layernorm_fwd(x, gmm, bta, y32, None, mean, rstd, M, H, drop=drop)
            return y32, None, mean, rstd
        y3 = torch.empty((M, 3 * H), dtype=BF16, device=x.device)       # the next GEMM's operand, written by the same kernel
        L.x3_layernorm_fwd(x, gmm, bta, y32, y3, mean, rstd, M, H, drop=drop)
        return y32, y3, mean, rstd

    def _ln3_bwd(self, dy, x, mean, rstd, key, dbias=None, drop=L.NO_DROP, out_drop=L.NO_DROP, m_dev=None, want3=True, want32=True,
                 dbias2=None):
        """-> (dx32: gradient w.r.t. the pre-LayerNorm sum, dxd3: its dropout-masked copy as a split operand).  Column sums
        (dgamma, dbeta, dbias [, dbias2]) are reduced by the grouped launch at the end of the block."""
        gmm, _, gg, gb = self.ln[key]
        M, H = x.shape
        dx32 = torch.empty((M, H), dtype=F32, device=x.device) if want32 else None
        dxd3 = torch.empty((M, 3 * H), dtype=BF16, device=x.device) if want3 else None
        part = torch.empty(self.part[H].numel(), dtype=F32, device=x.device)
        blocks = L.x3_layernorm_bwd_partials(dy, x, mean, rstd, gmm, dx32, dxd3, part, M, H, drop=drop, out_drop=out_drop, m_dev=m_dev)
        self._colsum(part, blocks, H, [gg, gb, dbias])
        if dbias2 is not None:
            self._colsum(part, blocks, H, [None, None, dbias2])
        return dx32, dxd3

    def _attn(self, q, k, v, mask, B, H, Tq, Tk, D, drop, save, qvar=None, kvar=None, tag=None):
        """-> (context fp32, context as a split operand, log-sum-exp)"""
        out = torch.empty((q.shape[0], H * D), dtype=F32, device=q.device)
        lse = torch.empty((B, H, Tq), dtype=F32, device=q.device) if save else None
        words, mq, mb = mask
        out3 = torch.empty((q.shape[0], 3 * _rup(H * D, 64)), dtype=BF16, device=q.device) if self.attn_planes else None
        L.x3_attn_fwd(q, k, v, out, lse, words, B, H, Tq, Tk, D, 1.0 / math.sqrt(D), mq, mb, drop, qvar=qvar, kvar=kvar, out3=out3)
        if out3 is None:
            out3 = self._split(out)
        if self.attn_sink is not None:          # diagnostic output (output_all_attention_masks): bf16-operand probabilities
            if qvar is not None or kvar is not None:
                raise RuntimeError("attention probabilities are collected on the padded schedule only")
            probs = torch.empty((B, H, Tq, Tk), dtype=F32, device=q.device)
            L.attn_probs(q.to(BF16), k.to(BF16), probs, words, B, H, Tq, Tk, D, 1.0 / math.sqrt(D), mq, mb, drop)
            self.attn_sink[tag] = probs
        return out, out3, lse

    # the shared-context pass's inference hooks (unimm_amd/engine.py) on fp32 rows and split operands
    def _ctx_rows(self, rows, width, device):
        """-> (context fp32, the same rows as a split operand | None): the two outputs of one attention launch"""
        out3 = torch.empty((rows, 3 * _rup(width, 64)), dtype=BF16, device=device) if self.attn_planes else None
        return torch.empty((rows, width), dtype=F32, device=device), out3

    def _attn_rows(self, q, k, v, ctx, mask, B, H, Tq, Tk, D, qvar=None, kvar=None, kshared=None):
        words, mq, mb = mask
        L.x3_attn_fwd(q, k, v, ctx[0], None, words, B, H, Tq, Tk, D, 1.0 / math.sqrt(D), mq, mb, L.NO_DROP, qvar=qvar, kvar=kvar,
                      out3=ctx[1], kshared=kshared)

    def _ctx_operand(self, ctx):
        return ctx[1] if ctx[1] is not None else self._split(ctx[0])

    def _embed_image(self, featd, locd, n, drop, save):
        """One GEMM over the split of [feat | loc | 0] with the w-type split of [W_feat | W_loc | 0], then LayerNorm."""
        F, Hv, dev = self.cfg.v_feature_size, self.cfg.v_hidden_size, featd.device
        packed32 = torch.zeros((n, self.vemb_k), dtype=F32, device=dev)
        packed32[:, :F].copy_(featd)
        packed32[:, F:F + 5].copy_(locd)
        packed3 = self._split(packed32)
        prev = torch.empty((n, Hv), dtype=F32, device=dev)
        L.gemm_nt(packed3, self.vemb_w3, prev, bias=self.vemb_b, M=n, N=Hv, K=3 * self.vemb_k)
        xv32, xv3, mv, rv = self._ln3(prev, "emb_v", save, drop=drop)
        if not save:
            return xv32, xv3, None
        A, v, K3 = self.arena, "bert.v_embeddings.", self.vemb_k

        def bwd(dxv):
            _, dpre3 = self._ln3_bwd(dxv, prev, mv, rv, "emb_v", dbias=A.grad(v + "image_embeddings.bias"), out_drop=drop,
                                     want32=False, dbias2=A.grad(v + "image_location_embeddings.bias"))
            self._wgrad3(dpre3, packed3, A.grad(v + "image_embeddings.weight"), n, Hv, F, Hv, K3)
            self._wgrad3(dpre3, packed3, A.grad(v + "image_location_embeddings.weight"), n, Hv, 5, Hv, K3, xcol0=F)
        return xv32, xv3, bwd

    def _embed_text(self, ids32, pos32, typ32, M, rows, drop, save, m_dev):
        H, dev = self.cfg.hidden_size, ids32.device
        scratch16 = torch.empty((M, H), dtype=BF16, device=dev)
        xt32 = torch.empty((M, H), dtype=F32, device=dev)
        emb = self._embed_text_args(ids32, pos32, typ32)
        L.embed_fwd(*emb, xt32, scratch16, M, H, self.cfg.type_vocab_size, drop=drop, m_dev=m_dev, rows=rows)
        del scratch16
        return xt32, self._split(xt32), (self._embed_text_bwd(L.embed_bwd_f32, emb, M, rows, drop, m_dev) if save else None)

    def _qkv_grad(self, qkv):
        """Gradient buffer of a fused projection output qkv (fp32 [rows, N], N % 64 == 0): with the matrix attention kernels a
        split operand [rows, 3 N] whose planes the attention backward fills directly, otherwise fp32 (split afterwards)."""
        if self.attn_planes:
            return torch.empty((qkv.shape[0], 3 * qkv.shape[1]), dtype=BF16, device=qkv.device)
        return torch.empty_like(qkv)

    def _proj(self, x3, lin):
        return self._lin3(x3, lin)

    def _proj_bwd(self, dqkv, x3, lin, add, m_dev=None):
        return self._lin3_bwd(dqkv if self.attn_planes else self._split(dqkv), x3, lin, m_dev=m_dev, add=add)

    def _attn_bwd(self, q, k, v, ctx, dctx, lse, mask, dq, dk, dv, N, B, H, Tq, Tk, D, drop, qvar=None, kvar=None):
        """dq / dk / dv: column slices [:, c0:c1] of `_qkv_grad` buffers (N = their projection width = the plane stride)."""
        delta = torch.empty_like(lse)
        words, mq, mb = mask
        L.x3_attn_bwd(q, k, v, ctx, dctx, lse, delta, dq, dk, dv, words, B, H, Tq, Tk, D, 1.0 / math.sqrt(D), mq, mb, drop,
                      qvar=qvar, kvar=kvar, planes=(N, dq.stride(0)) if self.attn_planes else None)

    # ------------------------------------------------------------------------------------------
    # blocks
    # ------------------------------------------------------------------------------------------
    def _post_attn(self, ctx3, res32, proj, ff1, ff2, ln_mid, ln_out, d_proj, d_ffn, save, m_dev=None):
        """The base engine's contract on split operands: ctx3 is the attention context as a split operand, the result is
        (y32, y3 split operand, bwd); bwd(dy) -> (dctx, dres), both fp32."""
        pre1 = self._lin3(ctx3, proj, L.EPI_BIAS_DROP_RESID, aux=res32, drop=d_proj)
        x1_32, x1_3, m1, r1 = self._ln3(pre1, ln_mid, save)
        u = self._lin3(x1_3, ff1)                                   # pre-activation, fp32
        h3 = self._op3(u, op=L.X3_GELU)[0]
        pre2 = self._lin3(h3, ff2, L.EPI_BIAS_DROP_RESID, aux=x1_32, drop=d_ffn)
        x2_32, x2_3, m2, r2 = self._ln3(pre2, ln_out, save)
        if not save:
            return x2_32, x2_3, None

        def bwd(dx2):
            dpre2, dpre2d3 = self._ln3_bwd(dx2, pre2, m2, r2, ln_out, dbias=ff2.gb, drop=d_ffn, m_dev=m_dev)
            du3 = self._op3(self._lin3_bwd(dpre2d3, h3, ff2, bias_grad=False, m_dev=m_dev), op=L.X3_MUL_DGELU, b=u)[0]
            dx1 = self._lin3_bwd(du3, x1_3, ff1, m_dev=m_dev, add=dpre2)
            dpre1, dpre1d3 = self._ln3_bwd(dx1, pre1, m1, r1, ln_mid, dbias=proj.gb, drop=d_proj, m_dev=m_dev)
            return self._lin3_bwd(dpre1d3, ctx3, proj, bias_grad=False, m_dev=m_dev), dpre1
        return x2_32, x2_3, bwd

    def _transform_head(self, x3, tr, ln_key, dec, ldo, save, M=None):
        """The base engine's contract on split operands; u (fp32) is returned whether or not save."""
        u = self._lin3(x3, tr, M=M)
        t = self._op3(u, op=L.X3_GELU, want3=False, want32=True)[1]
        _, hn3, mean, rstd = self._ln3(t, ln_key, save)
        return t, u, hn3, mean, rstd, self._lin3(hn3, dec, ldo=ldo)

    # ------------------------------------------------------------------------------------------
    # the step: the base engine's `_forward` / `_backward`, with fp32 gradient streams and split loss gradients
    # ------------------------------------------------------------------------------------------
    grad_dtype = F32
    prune_supported = False              # every block runs on all rows (this `_post_attn` takes no row list)

    def _forward(self, inp: dict, train: bool, save: bool, lm_rows: str, want_pred_v: bool):
        cfg = self.cfg
        if cfg.fixed_t_layer or cfg.fixed_v_layer or not cfg.with_coattention:
            raise NotImplementedError("fixed_t_layer / fixed_v_layer / with_coattention=False run on the bf16 engine only")
        return super()._forward(inp, train, save, lm_rows, want_pred_v)

    def _lm_loss_grad(self, lm, g_lm):
        n, dec = lm["n"], self.lin["dec"]
        dlog3 = torch.empty((n, 3 * dec.Np), dtype=BF16, device=self.arena.device)
        L.x3_lm_loss_bwd(lm["logits"], lm["labels"], lm["weights"], lm["lse"], self._gvec(g_lm), 1.0 / n, dlog3, n, self.cfg.vocab_size,
                         n_dev=lm.get("n_dev"), inv_dev=lm.get("inv_dev"))
        return dlog3

    def _img_loss_grad(self, img, gimg, rows):
        C = self.cfg.v_target_size
        dpred3 = torch.empty((rows, 3 * self.lin["imgdec"].Np), dtype=BF16, device=self.arena.device)
        if self.cfg.predict_feature:
            L.mse_loss_bwd(img["pred"], img["target"], img["label"], gimg, img["inv"], dpred3, rows, C, split=True)
        else:
            L.x3_kl_loss_bwd(img["pred"], img["target"], img["label"], img["lse"], gimg, img["inv"], dpred3, rows, C,
                             inv_dev=img.get("inv_dev"))
        return dpred3

    def _transform_head_bwd(self, dout3, hs, x3, tr, ln_key, dec, M=None, N=None, m_dev=None):
        dhn = self._lin3_bwd(dout3, hs["hn"], dec, M=M, m_dev=m_dev)       # dE += dlog^T hn ; dbias ; dhn = dlog @ E
        dt, _ = self._ln3_bwd(dhn, hs["t1"], hs["mean"], hs["rstd"], ln_key, m_dev=m_dev, want3=False)
        du3 = self._op3(dt, op=L.X3_MUL_DGELU, b=hs["u"])[0]
        return self._lin3_bwd(du3, x3, tr, m_dev=m_dev)

    def _rows_add(self, dst, idx, src, n):
        L.x3_rows_add(dst, idx, src, n, src.shape[1])
