"""Train-mode gradient yardstick -- TEST INFRASTRUCTURE shared by tests/test_grad_ref_cpu.py, tests/test_gpu_train_grads.py and
the train-mode tests of test_gpu_model.py / test_gpu_x3_model.py / test_gpu_trainer.py.

The engines never store a dropout mask: every site regenerates it from (seed, step, site name, coordinates), forward and
backward (unimm_amd/dropout.py).  `replay_drop_fn` restates that rule for the CPU oracle (oracle/vilbert_ref.py: `drop_fn`), so
that one oracle run in float64 gives the gradients a training step must produce, tensor by tensor:

  key          make_key(seed, step, crc32(site name))            (step = the engine's counter AFTER forward() bumped it)
  coordinates  (row, column) of the activation, rows numbered over all leading dimensions -- except at the text stream's
               row-wise sites (`is_text_rowwise`) of an unpadded step, whose rows are numbered over the VALID rows only
               (`packed_rows`: the engine's plan["rows"])
  scale        1 / (1 - p)

`sentinel_table` measures what a wrong mask at one site does to the gradients: the site's mask is replaced by the one of the
next step (same keep rate, other elements) and every tensor's relative L2 change is taken; the tensor that moves most is the
site's SENTINEL.  Half the smallest sentinel change is the gate under which a per-tensor relative-L2 check still sees every
site (tests/golden/dropout_sentinels.json, tests/test_grad_ref_cpu.py)."""
import json
import os
import zlib

import numpy as np
import torch

from oracle import plan_ref
from oracle import vilbert_ref as R
from unimm_amd import dropout as DR

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dropout_sentinels.json")
DEAD = 1e-6             # a tensor whose largest gradient element is below DEAD x the largest of all tensors is numerically zero
#                         (key biases: softmax is shift-invariant): bounded, not compared -- the rule of test_gpu_fullsize.py
DEAD_NORM_BOUND = 1e-3  # ... its norm stays below this share of the largest tensor norm


def load_table():
    """tests/golden/dropout_sentinels.json: {"key" | "coords": {site: {sentinel, change, max_norm_change}}} + how it was made."""
    with open(TABLE) as f:
        return json.load(f)


def gate(table=None):
    """G: half the smallest sentinel change of the committed table."""
    table = table or load_table()
    return 0.5 * min(e["change"] for kind in ("key", "coords") for e in table[kind].values())


def load_case(golden_dir, case, **switches):
    """Inputs of one golden on the small config (only its `in::` arrays are read), config switches applied
    -> (oracle config, seeded state dict, args, kw, config dict)."""
    with open(os.path.join(golden_dir, "small_config.json")) as f:
        cfgd = dict(json.load(f), **switches)
    ocfg = R.make_config(cfgd)
    g = np.load(os.path.join(golden_dir, case + ".npz"))
    i = lambda k: torch.from_numpy(np.ascontiguousarray(g["in::" + k]))
    kw = {k: i(k) for k in ("token_type_ids", "position_ids", "attention_mask", "image_attention_mask", "co_attention_mask",
                            "masked_lm_labels", "image_label", "image_target", "next_sentence_label", "nsp_weight", "lm_weight")}
    return ocfg, R.init_state_dict(ocfg, seed=11), (i("input_ids"), i("image_feat"), i("image_loc")), kw, cfgd


def site_names(cfg):
    """The dropout sites of one forward, by the names the engine and the oracle give them."""
    per = lambda prefix, n, subs: [f"{prefix}{i}.{s}" for i in range(n) for s in subs]
    names = ["emb_t", "emb_v", "fuse"]
    names += per("bert.encoder.layer.", cfg.num_hidden_layers, ("attn", "so", "out"))
    names += per("bert.encoder.v_layer.", cfg.v_num_hidden_layers, ("attn", "so", "out"))
    if cfg.with_coattention:
        names += per("bert.encoder.c_layer.", len(cfg.v_biattention_id), ("attn1", "attn2", "bo1", "bo2", "vout", "tout"))
    return sorted(names)


def is_text_rowwise(site):
    """Sites applied row by row to the text stream's [rows, hidden] activations: they follow the unpadded row numbering."""
    return site == "emb_t" or (site.startswith("bert.encoder.layer.") and site.endswith((".so", ".out"))) \
        or site.endswith((".bo2", ".tout"))


def packed_rows(attention_mask, co_attention_mask=None, masked_lm_labels=None, lm_weight=None):
    """Flat indices (b * T + t) of the text rows an unpadded step computes, in order: the valid PREFIX of every sequence as
    include/unimm_hip.h defines it (oracle/plan_ref.py: a token is valid when it attends something, is attended by a token or
    a region, or carries a label / weight).  int64 tensor."""
    np_ = lambda x: None if x is None else np.asarray(x)
    am = np_(attention_mask)
    B, T = am.shape[0], am.shape[-1]
    lens = plan_ref.lengths(am, np_(co_attention_mask), np_(masked_lm_labels), np_(lm_weight), None, B, T)[:B]
    return torch.from_numpy(np.concatenate([np.arange(b * T, b * T + int(n), dtype=np.int64) for b, n in enumerate(lens)]))


def replay_drop_fn(seed, step, rows, mutate=None, coords_rows=None):
    """-> drop_fn(site, x, p) for oracle.vilbert_ref.forward that applies the engines' masks of (seed, step).
    rows: `packed_rows(...)` of an unpadded step, None = padded coordinates everywhere.
    mutate: {site: kind} deliberately breaks one site -- "key": the mask of step + 1; "coords" (text row-wise sites only):
    padded coordinates where packed ones belong and the other way round (packed ones from `coords_rows` when rows is None);
    "bwd": the right mask in the forward pass and the mask of step + 1 in the backward pass (a backward that regenerates its
    mask from other arguments than its forward).
    drop_fn.sites lists the sites it was called for, in call order."""
    mutate = dict(mutate or {})
    for s, kind in mutate.items():
        if kind not in ("key", "coords", "bwd") or (kind == "coords" and not is_text_rowwise(s)):
            raise ValueError(f"no mutation {kind!r} for site {s!r}")
    as_rows = lambda r: None if r is None else torch.as_tensor(r).detach().cpu().long().reshape(-1)
    rows, coords_rows = as_rows(rows), as_rows(coords_rows)
    seen = []

    def drop_fn(site, x, p):
        seen.append(site)
        kind = mutate.get(site)
        if kind == "bwd":
            fwd, bwd = (mask(site, x, p, None, step + d) for d in (0, 1))
            return _MaskFwdBwd.apply(x, fwd, bwd)
        return x * mask(site, x, p, kind, step)

    def mask(site, x, p, kind, step):
        key = DR.make_key(seed, step + 1 if kind == "key" else step, zlib.crc32(site.encode()) & 0xFFFFFFFF)
        _, thr, scale = DR.drop_arg(p, key)
        use = rows if is_text_rowwise(site) else None
        if kind == "coords":
            use = None if use is not None else (coords_rows if coords_rows is not None else rows)
            if use is None and rows is None:
                raise ValueError("the 'coords' mutation of a padded replay needs coords_rows")
        if use is not None:                     # device coordinates: (packed row, column); rows outside the plan are never computed
            n = x.shape[-1]
            keep = torch.ones((x.numel() // n, n), dtype=torch.bool)
            keep[use] = torch.from_numpy(DR.keep_mask2d(key, thr, use.numel(), n))
            keep = keep.view(x.shape)
        else:
            keep = torch.from_numpy(DR.keep_mask_nd(key, thr, tuple(x.shape)))
        return keep.to(x.dtype) * scale          # (in x's own type: the oracle may run in double)

    drop_fn.sites = seen
    return drop_fn


class _MaskFwdBwd(torch.autograd.Function):
    """x * fwd in the forward pass, g * bwd in the backward pass."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.save_for_backward(bwd)
        return x * fwd

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


def oracle_grads(sd, ocfg, args, kw, drop_fn, dtype=torch.float64, objective=None):
    """One oracle forward + backward in `dtype` -> (losses {lm_loss, img_loss, nsp_loss}, NSP scores, {name: gradient | None}).
    objective(out) -> scalar; default: the sum of the three losses.  The tied decoder weight is the word-embedding leaf, as in
    the model (its gradient is listed under the word embeddings only)."""
    cast = lambda v: v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k != R.TIED[0]}
    leaves[R.TIED[0]] = leaves[R.TIED[1]]
    out = R.forward(leaves, ocfg, *[cast(a) for a in args], **{k: cast(v) for k, v in kw.items()}, drop_fn=drop_fn)
    loss = (out["lm_loss"] + out["img_loss"] + out["nsp_loss"]).sum() if objective is None else objective(out)
    loss.backward()
    losses = {k: out[k].detach() for k in ("lm_loss", "img_loss", "nsp_loss")}
    return losses, out["nsp"].detach(), {n: p.grad for n, p in leaves.items() if n != R.TIED[0]}


def compare(got, want):
    """got / want: {name: gradient | None} -> {name: dict(l2, norm_err, max_err, dead, norm, want_norm)} over the tensors with a
    gradient on both sides, in float64.  l2 = ||got - want|| / ||want||, norm_err = | ||got|| - ||want|| | / ||want||,
    max_err = max |got - want| / max |want|; a dead tensor (see DEAD) carries only its norms."""
    live = {n: w.detach().double().cpu() for n, w in want.items() if w is not None and got.get(n) is not None}
    gmax = max(float(w.abs().max()) for w in live.values())
    res = {}
    for n, w in live.items():
        g = got[n].detach().double().cpu()
        wn, gn = float(w.norm()), float(g.norm())
        if float(w.abs().max()) < DEAD * gmax:
            res[n] = dict(dead=True, norm=gn, want_norm=wn)
            continue
        res[n] = dict(dead=False, norm=gn, want_norm=wn, l2=float((g - w).norm()) / wn, norm_err=abs(gn - wn) / wn,
                      max_err=float((g - w).abs().max() / w.abs().max()))
    return res


def family(name):
    """Tensor family for the printed tables: one encoder block, or the first two name parts."""
    p = name.split(".")
    return ".".join(p[2:4]) if name.startswith("bert.encoder") else ".".join(p[:2])


def sentinel_table(sd, ocfg, args, kw, seed, step, rows, sites, kind="key", dtype=torch.float64, base=None):
    """The base replay, then one oracle run per site with that site mutated -> (table, base gradients);
    table = {site: (sentinel tensor, its change ||g_mut - g|| / ||g||, largest | ||g_mut|| - ||g|| | / ||g|| of any tensor)}."""
    if base is None:
        base = oracle_grads(sd, ocfg, args, kw, replay_drop_fn(seed, step, rows), dtype)[2]
    table = {}
    for s in sites:
        mut = oracle_grads(sd, ocfg, args, kw, replay_drop_fn(seed, step, rows, {s: kind}), dtype)[2]
        c = {n: v for n, v in compare(mut, base).items() if not v["dead"]}
        name = max(c, key=lambda n: c[n]["l2"])
        table[s] = (name, c[name]["l2"], max(v["norm_err"] for v in c.values()))
    return table, base
