"""Information flow through both engines, in bits: an output that tests/flow_ref.py's closure does not connect to an input must
come back BIT-IDENTICAL when that input changes at unchanged shapes, and an output of the one-layer closure must change.  With
the shapes the step plan, every tile choice, every dropout counter and every launch are unchanged, so nothing is compared
through a tolerance; the only looseness is `== 0` for gradient rows that must be zero (-0 is legitimate).

Small config, T = 64, R = 37, B <= 12, engines bf16 and fp32x3 (fp32x3 without the options it does not have: `lazy_ln`, the
pruned last text layer, answer generation, shared-context training).  Bits are taken as tests/test_gpu_row_edges.py takes them.

Baseline: every case first runs its unperturbed input TWICE and requires all compared outputs to repeat bit for bit.  One option
is pinned for that: `engine.splitk = False` -- `unimm_gemm_nt` with more than two K splits adds its partial tiles in arrival
order.  Weight gradients (fp32 atomic sums) do not repeat, so the backward checks use exact zeros and, for the shared-context
step, the gradient arena that tests/test_gpu_shared_training.py establishes as reproducible.
What this file found: the per-sequence likelihood did not repeat.  `unimm_segment_sum` added every labelled row to its
sequence's score with an atomic of its own, so a score of three or more rows took the bits of the threads' arrival order -- the
baseline of checks 1, 4 and 5 failed on it with every other output identical.  No option pins that launch; the kernel now adds
the rows of a sequence in row order and issues one atomic per run (unimm_amd/csrc/loss.hip), and the scores repeat.

Forward checks (eval mode, and train mode with dropout under a fixed (seed, step)); per case the counts printed are the outputs
compared bit for bit outside the closure (>= 8 required) and the ones inside that must and do change (>= 4 required):
 1 isolation      sequence j's tokens, type ids and image features replaced by others at the same length and masks: every other
                  sequence's sequence-output rows, labelled-row LM scores and losses, NSP logits, image predictions and likelihood
                  identical, j's own changed.  unpad x prune_last_text x lazy_ln x compact inputs (DialogMaskSpec + image_index;
                  images are then shared between sequences, so the text alone is replaced).
 2 padding        loud token / position / type ids past every sequence's length, loud features and boxes in masked regions, and
                  the mask bits of dead query rows set: co-attention rows of masked regions always; text-mask rows past the length
                  only with unpad = False -- PRECONDITION NARROWED: with unpad = True the plan (include/unimm_hip.h) defines a row
                  that attends something as valid, so such a bit legitimately lengthens the sequence and changes the shapes.
 3 causality      generative mode, answer token k changed (the input token; labels stay): context rows, image stream, copy rows
                  <= k and their likelihood terms (row-sparse `lm` output) identical, copy row k + 1 changed.  k = 0, the last
                  token, a 1-token answer.
 4 permutation    sequences permuted (eval, unpad = True, attn_longest_first on and off): per-sequence outputs permute bit-exactly.
 5 shared scoring `sequence_log_likelihood(shared_context=)`, bare list and SharedContext(ids, 64), 3 rounds x 5 options.
 6 generation     `generate_answers(beams=1)` and `(samples=2)`, 4 dialogs: another dialog's context changed.
Backward checks:
 7 dead positions every text row gets a position id of its own (b * T + t < 512), so the rows of position_embeddings.weight.grad
                  are the input rows' gradients: rows that no loss-bearing output reaches backwards (flow_ref) are exactly 0, the
                  others are not; discriminative batch with a long sequence that carries no loss (then given a label), and a
                  generative batch.
 8 shared step    `forward_backward(shared_context=)`: an answer with zero weight (lm_weight 0 / advantage 0) replaced by another:
                  loss and gradient arena bit-identical; with the weight restored they differ.

Does each check bite?  Three edits tried by hand on a scratch copy, on an MI355X, and not kept:
 * `_prune_rows` handing the pruned layer its labelled `rows` rolled by one entry: checks 1 (dense, prune) and 3 fail; check 2,
   which does not prune, passes.
 * one co-attention bit set past every sequence's length in the words `unimm_mask_synth` returns (`_prep_masks`): check 2
   (compact) fails; check 1 (compact) passes -- the bit makes a row read its OWN sequence's padding, not a neighbour.
 * `ks_len` of the shared pass dropped by one (`_forward_shared`): NOT caught here -- checks 5 and 8 pass.  The edit removes
   an edge instead of adding one: the candidates lose a context key, but every remaining path is inside the closure and the last
   context row still reaches them through the other context rows, so nothing leaks and everything that must change does.  A
   missing edge is a numerical error, which is what the tolerance tests against per-candidate scoring are for."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import masks as OM
from tests import flow_ref as FR
from tests.test_gpu_row_edges import bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "small_config.json")
T, NREG, MASK = 64, 37, 103
MIN_OUT, MIN_IN = 8, 4
ENGINES = ("bf16", "fp32x3")
TEXT_KINDS = ("seq", "lm", "nll")
KEYS = ("token_type_ids", "position_ids", "attention_mask", "image_attention_mask", "co_attention_mask", "masked_lm_labels",
        "lm_weight", "image_index", "image_label", "image_target", "next_sentence_label", "nsp_weight")
_MODELS = {}


def build(compute):
    """one model per engine for the whole file (weights of the oracle's seeded generator), split-K pinned off"""
    if compute not in _MODELS:
        from oracle import vilbert_ref as R
        from unimm_amd import BertConfig, BertForMultiModalPreTraining
        cfgd = json.load(open(CFG))
        model = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd), compute_dtype=compute)
        sd = R.init_state_dict(R.make_config(cfgd), seed=11)
        sd["cls.predictions.bias"] = torch.randn(sd["cls.predictions.bias"].shape, generator=torch.Generator().manual_seed(5)) * 3.0
        model.load_state_dict(sd, strict=True)
        model = model.cuda()
        model.engine.splitk = False
        _MODELS[compute] = model
    return _MODELS[compute]


def configure(model, unpad=True, prune=True, lazy=True, longest=True):
    eng = model.engine
    eng.ensure(torch.device("cuda", 0))
    eng.unpad, eng.prune_last_text, eng.attn_longest_first, eng.splitk = unpad, prune, longest, False
    if model.compute_dtype == "bf16":
        eng.lazy_ln = lazy
    return eng


def schedules(compute):
    """(unpad, prune, lazy) an engine has"""
    if compute == "bf16":
        return [(u, p, z) for u in (True, False) for p in (True, False) for z in (True, False)]
    return [(u, False, False) for u in (True, False)]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def dense_masks_of(b):
    """CPU dense masks of a batch, whichever way it carries them -> (text [B, T, T], image [B, R], co [B, R, T] or [B, T])"""
    am = b["attention_mask"]
    if torch.is_tensor(am):
        return am.cpu(), b["image_attention_mask"].cpu(), b["co_attention_mask"].cpu()
    txt, co = am.dense(T)
    im = b["image_attention_mask"].cpu()
    return txt, im, co


def describe(model, b):
    """closures and the valid rows of a batch"""
    am, im, co = dense_masks_of(b)
    full, near = FR.closure(am, im, co, model.config), FR.one_layer(am, im, co, model.config)
    lens = FR.valid_lengths(am, co, b["masked_lm_labels"].cpu())
    valid_t = np.arange(T)[None, :] < lens[:, None]
    return SimpleNamespace(full=full, near=near, lens=lens, valid_t=valid_t, valid_v=im.numpy() != 0, B=len(lens))


def synth_batch(model, compact, seed=5, n_seq=12):
    from unimm_amd import synth
    b = synth.make_batch(n_seq=n_seq, T=T, R=NREG, cfg=model.config, seed=seed, device="cuda", compact=compact)
    b["position_ids"] = b.pop("token_position_ids")
    if compact:
        b["attention_mask"], b["co_attention_mask"] = b.pop("mask_spec"), None
        b["image_feat"], b["image_loc"], b["image_target"] = (b.pop(k + "_unique") for k in ("image_feat", "image_loc", "image_target"))
    return b


def gen_batch(answers=(5, 1, 3, 8, 2, 5), contexts=((4, 3, 5), (6, 2), (3, 3, 3, 2), (9, 4), (2, 7, 3), (5, 5, 5, 4)), seed=17,
              F=192, C=101):
    """generative sequences from oracle/masks.py, labels on the copy rows only -> (batch on the device, [(c, L, n)])"""
    rng = np.random.default_rng(seed)
    rows, info = [], []
    for a, ctx in zip(answers, contexts):
        utts = [rng.integers(110, 1000, size=n).tolist() for n in tuple(ctx) + (a,)]
        rows.append(OM.encode_gen(utts, start_segment=int(rng.integers(0, 2)), max_seq_len=T))
        L = 1 + sum(n + 1 for n in ctx) + a + 1
        info.append((L - (a + 1), L, a + 1))
        assert L + a + 1 <= T
    B = len(rows)
    cat = lambda k: torch.from_numpy(np.concatenate([r[k] for r in rows]))
    tgt = rng.random((B, NREG, C)).astype(np.float32)
    label = np.where(rng.random((B, NREG)) < 0.2, 1, -1)
    label[:, 0] = 0
    b = dict(input_ids=cat("tokens"), token_type_ids=cat("segments"), position_ids=cat("positions"), masked_lm_labels=cat("labels"),
             lm_weight=cat("weights"), attention_mask=cat("txt_attention_mask").bool(),
             co_attention_mask=cat("co_attention_mask").bool()[:, None, :].expand(B, NREG, T).contiguous(),
             image_attention_mask=torch.ones(B, NREG), image_feat=torch.from_numpy(np.maximum(rng.standard_normal((B, NREG, F)), 0).astype(np.float32)),
             image_loc=torch.from_numpy(rng.random((B, NREG, 5)).astype(np.float32)),
             image_target=torch.from_numpy(tgt / tgt.sum(-1, keepdims=True)), image_label=torch.from_numpy(label.astype(np.int64)),
             next_sentence_label=torch.zeros(B, dtype=torch.int64), nsp_weight=torch.tensor([[1.0, 1.0]]))
    return {k: v.cuda() for k, v in b.items()}, info


def clone(b, *keys):
    p = dict(b)
    for k in keys:
        p[k] = b[k].clone()
    return p


# ---------------------------------------------------------------------------------------------------------------------
# running and comparing
# ---------------------------------------------------------------------------------------------------------------------
def run(model, b, d, train, want_seq, likelihood=False):
    """One engine forward at a fixed (seed, step) -> {kind: (flat positions, bits [N, width])}: seq (fp32 sequence-output rows),
    lm / nll (the labelled rows' logits and loss terms), img (image prediction rows), nsp, ll (sequence_log_likelihood).
    Text kinds are indexed b * T + t, img b * R + r, nsp and ll b.  Only rows anybody reads: valid rows, unmasked regions.
    want_seq=False: the training step's call (save=True), whose last text layer may run on the loss rows only."""
    eng = model.engine
    eng.seed, eng.step = 1234, 5
    V, C = model.config.vocab_size, model.config.v_target_size
    inp = dict(input_ids=b["input_ids"], image_feat=b["image_feat"], image_loc=b["image_loc"], **{k: b.get(k) for k in KEYS})
    with torch.no_grad():
        out = eng.forward(inp, train=train, save=not want_seq, lm_rows="labelled", want_pred_v=True, want_seq=want_seq)
        B = out["B"]
        lm = out["lm"]
        pos = lm["pos_idx"].long().cpu().numpy()
        n = len(pos)
        res = dict(lm=(pos, bits(lm["logits"][:n, :V])), nll=(pos, bits(lm["rownll"][:n].reshape(n, 1))))
        if out.get("pruned") is None:
            rows = np.nonzero(d.valid_t.reshape(-1))[0]
            res["seq"] = (rows, bits(eng.padded(out, out["seq32_t"]).view(B * T, -1).float())[rows])
        else:
            res["seq"] = (np.concatenate([np.arange(B) * T, pos]), bits(out["seq32_t"][:B + n].float()))
        regions = np.nonzero(d.valid_v.reshape(-1))[0]
        res["img"] = (regions, bits(out["pred_v"][:, :, :C].reshape(B * NREG, C).float())[regions])
        res["nsp"] = (np.arange(B), bits(out["nsp"].float()))
        pruned = out.get("pruned") is not None
        del out, lm
        if likelihood:
            kw = {k: b.get(k) for k in KEYS[:5] + ("image_index",)}
            ll, _ = model.sequence_log_likelihood(b["input_ids"], b["image_feat"], b["image_loc"], b["masked_lm_labels"], **kw)
            res["ll"] = (np.arange(B), bits(ll.reshape(B, 1)))
    torch.cuda.synchronize()
    return res, pruned


def reach(flow_sets, B):
    """per-sequence reach dicts {b: from_*()} -> {kind: flat boolean array over the kind's index space}"""
    t, v, s = np.zeros((B, T), bool), np.zeros((B, NREG), bool), np.zeros(B, bool)
    for b, r in flow_sets.items():
        t[b] |= r["text"]
        v[b] |= r["regions"]
        s[b] |= r["nsp"]
    return t, v, s


def sets_of(flow_sets, d, labels):
    t, v, s = reach(flow_sets, d.B)
    ll = (t & (labels.cpu().numpy() != -1)).any(1)
    return dict(seq=t.reshape(-1), lm=t.reshape(-1), nll=t.reshape(-1), img=v.reshape(-1), nsp=s, ll=ll)


def same_bits(what, a, b):
    for k in a:
        assert np.array_equal(a[k][0], b[k][0]), (what, k)
        diff = (a[k][1] != b[k][1]).reshape(len(a[k][0]), -1).any(1)
        assert not diff.any(), f"{what}: {k} does not repeat at {a[k][0][diff][:8].tolist()}"


def check(what, base, new, inside, must):
    """everything outside `inside` bit-identical, everything in `must` changed, with the counts that keep it from being vacuous"""
    n_out = n_in = 0
    for k in base:
        pos = base[k][0]
        assert np.array_equal(pos, new[k][0]), (what, k)
        diff = (base[k][1] != new[k][1]).reshape(len(pos), -1).any(1)
        leak = diff & ~inside[k][pos]
        assert not leak.any(), f"{what}: {k} outside the closure changed at {pos[leak][:12].tolist()} ({int(leak.sum())} rows)"
        still = must[k][pos] & ~diff
        assert not still.any(), f"{what}: {k} inside the closure did not change at {pos[still][:12].tolist()}"
        n_out += int((~inside[k][pos]).sum())
        n_in += int(must[k][pos].sum())
    print(f"    {what}: {n_out} outputs compared bit for bit outside the closure, {n_in} inside required to change")
    assert n_out >= MIN_OUT and n_in >= MIN_IN, (what, n_out, n_in)


def modes():
    return (("eval", False), ("train", True))


# ---------------------------------------------------------------------------------------------------------------------
# 1 isolation
# ---------------------------------------------------------------------------------------------------------------------
def replace_sequence(b, j, length, rng, image):
    p = clone(b, "input_ids", "token_type_ids", *(("image_feat", "image_loc") if image else ()))
    ids = p["input_ids"][j, :length]
    new = torch.from_numpy(rng.integers(110, 1000, size=length)).to(ids.device)
    p["input_ids"][j, :length] = torch.where(ids == MASK, ids, new)
    p["token_type_ids"][j, :length] = 1 - b["token_type_ids"][j, :length]
    if image:
        f = b["image_feat"][j]
        p["image_feat"][j] = torch.from_numpy(np.maximum(rng.standard_normal(tuple(f.shape)), 0).astype(np.float32)).to(f.device)
        p["image_loc"][j, 1:] = 1.0 - b["image_loc"][j, 1:]
    return p


@pytest.mark.parametrize("compact", [False, True], ids=["dense", "compact"])
@pytest.mark.parametrize("compute", ENGINES)
def test_isolation(compute, compact):
    model = build(compute)
    b = synth_batch(model, compact)
    d = describe(model, b)
    spec_modes = (b["attention_mask"].mode if compact else None)
    rng = np.random.default_rng(1)
    print()
    for unpad, prune, lazy in schedules(compute):
        configure(model, unpad, prune, lazy)
        for mname, train in modes():
            want_seq = not prune
            what = f"{compute} {'compact' if compact else 'dense'} unpad={unpad} prune={prune} lazy_ln={lazy} {mname}"
            base, pruned = run(model, b, d, train, want_seq, likelihood=not train)
            assert pruned == (prune and compute == "bf16"), what
            same_bits(what + " baseline", base, run(model, b, d, train, want_seq, likelihood=not train)[0])
            for j in (1, 8):
                p = replace_sequence(b, j, int(d.lens[j]), rng, image=not compact)
                new, _ = run(model, p, d, train, want_seq, likelihood=not train)
                inside = sets_of({j: d.full.from_sequence(j, regions=not compact)}, d, b["masked_lm_labels"])
                must = sets_of({j: d.near.from_sequence(j, regions=not compact)}, d, b["masked_lm_labels"])
                check(f"{what} j={j}", base, new, inside, must)
    assert spec_modes is None or len(spec_modes) == d.B


# ---------------------------------------------------------------------------------------------------------------------
# 2 padding content
# ---------------------------------------------------------------------------------------------------------------------
def loud_padding(b, d, rng, text_mask_rows):
    dense = torch.is_tensor(b["attention_mask"])
    keys = ["input_ids", "token_type_ids", "position_ids"] + (["image_feat", "image_loc", "co_attention_mask"] if dense else [])
    if dense and text_mask_rows:
        keys.append("attention_mask")
    p = clone(b, *keys)
    n_loud = 0
    for s in range(d.B):
        n = int(d.lens[s])
        k = T - n
        if k:
            p["input_ids"][s, n:] = torch.from_numpy(rng.integers(110, 1000, size=k)).cuda()
            p["position_ids"][s, n:] = torch.from_numpy(rng.integers(1, 512, size=k)).cuda()
            p["token_type_ids"][s, n:] = 1
            n_loud += k
            if dense and text_mask_rows:
                p["attention_mask"][s, n:, :n] = True         # dead query rows reading live keys
        dead = np.nonzero(~d.valid_v[s])[0]
        if dense and len(dead):
            ix = torch.from_numpy(dead).cuda()
            p["image_feat"][s, ix] = b["image_feat"][s, ix] * -30.0 + 100.0
            p["image_loc"][s, ix] = 7.0
            p["co_attention_mask"][s, ix, :n] = True          # a masked region's own query row
            n_loud += len(dead)
    return p, n_loud


@pytest.mark.parametrize("compact", [False, True], ids=["dense", "compact"])
@pytest.mark.parametrize("compute", ENGINES)
def test_padding_content(compute, compact):
    model = build(compute)
    b = synth_batch(model, compact, seed=6)
    if not compact:
        b["image_attention_mask"] = b["image_attention_mask"].clone()
        b["image_attention_mask"][2, 30:] = 0
        b["image_attention_mask"][7, 11:] = 0
        b["image_attention_mask"][9, 36:] = 0
    d = describe(model, b)
    rng = np.random.default_rng(2)
    print()
    for unpad in (True, False):
        configure(model, unpad, prune=False)
        p, n_loud = loud_padding(b, d, rng, text_mask_rows=not unpad)
        assert n_loud >= MIN_OUT
        for mname, train in modes():
            what = f"{compute} {'compact' if compact else 'dense'} unpad={unpad} {mname}"
            base, _ = run(model, b, d, train, True, likelihood=not train)
            same_bits(what + " baseline", base, run(model, b, d, train, True, likelihood=not train)[0])
            new, _ = run(model, p, d, train, True, likelihood=not train)
            same_bits(what, base, new)
            n = sum(len(v[0]) for v in base.values())
            print(f"    {what}: {n_loud} loud dead positions, {n} valid outputs compared bit for bit")
            assert n >= MIN_OUT


# ---------------------------------------------------------------------------------------------------------------------
# 3 causality
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ENGINES)
def test_causality(compute):
    model = build(compute)
    b, info = gen_batch()
    d = describe(model, b)
    print()
    cases = [("k=0", 0, 0), ("last token", 3, 7), ("1-token answer", 1, 0)]
    for want_seq in ((True, False) if compute == "bf16" else (True,)):
        configure(model)
        for mname, train in modes():
            base, pruned = run(model, b, d, train, want_seq, likelihood=not train)
            assert pruned == (not want_seq)
            same_bits(f"{compute} {mname} baseline", base, run(model, b, d, train, want_seq, likelihood=not train)[0])
            for cname, s, k in cases:
                c, L, n = info[s]
                assert k <= n - 2
                p = clone(b, "input_ids")
                p["input_ids"][s, c + k] = 110 + (int(b["input_ids"][s, c + k]) + 333) % 800
                new, _ = run(model, p, d, train, want_seq, likelihood=not train)
                inside = sets_of({s: d.full.from_text(s, c + k)}, d, b["masked_lm_labels"])
                must = sets_of({s: d.near.from_text(s, c + k)}, d, b["masked_lm_labels"])
                for kind in TEXT_KINDS:      # what the closure must say for this to be the causality check
                    flat = inside[kind].reshape(d.B, T)
                    assert not flat[s, 1:c + k].any() and not flat[s, L:L + k + 1].any() and must[kind].reshape(d.B, T)[s, L + k + 1]
                assert not inside["img"].any()
                for x in (inside, must):     # rows nobody reads are not compared
                    for kind in TEXT_KINDS:
                        x[kind] = x[kind] & d.valid_t.reshape(-1)
                check(f"{compute} {mname} {'all rows' if want_seq else 'loss rows'} {cname}", base, new, inside, must)


# ---------------------------------------------------------------------------------------------------------------------
# 4 batch permutation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ENGINES)
def test_batch_permutation(compute):
    model = build(compute)
    b = synth_batch(model, False, seed=8)
    d = describe(model, b)
    perm = np.array([5, 0, 11, 3, 9, 1, 7, 2, 10, 4, 6, 8])
    ix = torch.from_numpy(perm).cuda()
    p = {k: (v.index_select(0, ix) if torch.is_tensor(v) and v.dim() and v.shape[0] == d.B else v) for k, v in b.items()}
    dp = describe(model, p)
    assert dp.lens.tolist() == d.lens[perm].tolist() and sorted(perm.tolist()) == list(range(d.B)) and d.lens.sum() < d.B * T
    strides = dict(seq=T, lm=T, nll=T, img=NREG, nsp=1, ll=1)
    print()
    for longest in (True, False):
        configure(model, unpad=True, prune=False, longest=longest)
        base, _ = run(model, b, d, False, True, likelihood=True)
        same_bits("baseline", base, run(model, b, d, False, True, likelihood=True)[0])
        new, _ = run(model, p, dp, False, True, likelihood=True)
        n = 0
        for k, (pos, val) in new.items():
            S = strides[k]
            old = perm[pos // S] * S + pos % S               # sequence i of the permuted batch is sequence perm[i]
            where = {int(q): i for i, q in enumerate(base[k][0])}
            rows = np.array([where[int(q)] for q in old])
            diff = (val != base[k][1][rows]).reshape(len(pos), -1).any(1)
            assert not diff.any(), f"{compute} longest_first={longest}: {k} of permuted sequences {sorted(set((pos[diff] // S).tolist()))} differ"
            n += len(pos)
        print(f"    {compute} attn_longest_first={longest}: {n} per-sequence outputs permute bit for bit")
        assert n >= MIN_OUT


# ---------------------------------------------------------------------------------------------------------------------
# 5 shared-context scoring
# ---------------------------------------------------------------------------------------------------------------------
def scoring_case(model):
    from unimm_amd import synth
    b = synth.make_scoring_batch(rounds=3, options=5, T=T, cfg=model.config, seed=7, a_range=(1, 6), c_range=(8, 30), device="cuda")
    spec = b.pop("mask_spec")
    c, n = spec.length - spec.answer, spec.answer
    return b, b.pop("context_group"), c, n


def shared_scores(model, b, groups):
    kw = dict(token_type_ids=b["token_type_ids"], position_ids=b["token_position_ids"], attention_mask=b["attention_mask"],
              co_attention_mask=b["co_attention_mask"], image_attention_mask=b["image_attention_mask"])
    with torch.no_grad():
        sc, nsp = model.sequence_log_likelihood(b["input_ids"], b["image_feat"], b["image_loc"], b["masked_lm_labels"],
                                                shared_context=groups, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sc).all())
    return bits(sc.reshape(-1, 1)), bits(nsp.float())


@pytest.mark.parametrize("form", ["list", "SharedContext"])
@pytest.mark.parametrize("compute", ENGINES)
def test_shared_context_scoring(compute, form):
    from unimm_amd.scoring import SharedContext
    model = build(compute).eval()
    configure(model)
    b, grp, c, n = scoring_case(model)
    B = len(c)
    groups = grp if form == "list" else SharedContext(grp, 64)
    sc0, nsp0 = shared_scores(model, b, groups)
    sc1, nsp1 = shared_scores(model, b, groups)
    assert np.array_equal(sc0, sc1) and np.array_equal(nsp0, nsp1), "baseline does not repeat"
    rows = lambda x, y: (x != y).reshape(B, -1).any(1)
    print()
    # (a) two candidates (of different rounds) get other answers of the same length: tokens and the copy rows' labels
    picked = [1, 8]
    p = clone(b, "input_ids", "masked_lm_labels")
    for a in picked:
        L = int(c[a] + n[a])
        ans = 110 + (b["input_ids"][a, c[a]:L - 1] + 77) % 800
        p["input_ids"][a, c[a]:L - 1] = ans
        p["masked_lm_labels"][a, L:L + n[a] - 1] = ans
    sc, nsp = shared_scores(model, p, groups)
    other = np.array([q not in picked for q in range(B)])
    ds, dn = rows(sc0, sc), rows(nsp0, nsp)
    assert not ds[other].any() and not dn[other].any(), (np.nonzero(ds & other)[0], np.nonzero(dn & other)[0])
    assert ds[~other].all() and dn[~other].all()
    print(f"    {compute} {form} answers of {picked}: {2 * int(other.sum())} scores and NSP rows bit-identical, {2 * len(picked)} changed")
    assert 2 * int(other.sum()) >= MIN_OUT and 2 * len(picked) >= MIN_IN
    # (b) one round's context changes (in every member: it is shared)
    r = 1
    members = np.nonzero(grp.cpu().numpy() == r)[0]
    p = clone(b, "input_ids")
    p["input_ids"][members, 2] = 110 + (b["input_ids"][members, 2] + 55) % 800
    sc, nsp = shared_scores(model, p, groups)
    other = np.ones(B, bool)
    other[members] = False
    ds, dn = rows(sc0, sc), rows(nsp0, nsp)
    assert not ds[other].any() and not dn[other].any(), (np.nonzero(ds & other)[0], np.nonzero(dn & other)[0])
    assert ds[members].all(), np.nonzero(~ds & ~other)[0]
    print(f"    {compute} {form} context of round {r}: {2 * int(other.sum())} scores and NSP rows bit-identical, {len(members)} scores changed")
    assert 2 * int(other.sum()) >= MIN_OUT and len(members) >= MIN_IN
    # (c) the candidates permuted within their groups
    perm = np.array([3, 0, 4, 1, 2, 9, 8, 7, 6, 5, 11, 12, 10, 14, 13])
    assert (grp.cpu().numpy()[perm] == grp.cpu().numpy()).all()
    ix = torch.from_numpy(perm).cuda()
    p = {k: v.index_select(0, ix) for k, v in b.items()}
    sc, nsp = shared_scores(model, p, groups)
    assert np.array_equal(sc, sc0[perm]), np.nonzero(rows(sc, sc0[perm]))[0]
    assert np.array_equal(nsp, nsp0[perm]), np.nonzero(rows(nsp, nsp0[perm]))[0]
    print(f"    {compute} {form} candidates permuted within their groups: {2 * B} scores and NSP rows permute bit for bit")


# ---------------------------------------------------------------------------------------------------------------------
# 6 generation cache
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(beams=1), dict(samples=2, seed=3, temperature=0.9)], ids=["beams1", "samples2"])
def test_generation_neighbour_context(kw):
    from tests.test_gpu_generate import gen_kwargs, make_dialogs
    model = build("bf16").eval()
    configure(model)
    G, g = 4, 2
    d, c, _ = make_dialogs(G, T, 1000, NREG, 192, seed=12, cmin=8, cmax=30)

    def gen(dd):
        res = model.generate_answers(dd["input_ids"], dd["image_feat"], dd["image_loc"], c, max_answer_len=8, min_answer_len=3,
                                     **gen_kwargs(dd), **kw)
        torch.cuda.synchronize()
        names = [k for k in ("tokens", "lengths", "scores", "logp", "step_logp", "step_logq") if getattr(res, k, None) is not None]
        return {k: getattr(res, k).detach().cpu().reshape(G, -1) for k in names}

    base, again = gen(d), gen(d)
    for k in base:
        assert torch.equal(base[k], again[k]) or np.array_equal(bits(base[k].float()), bits(again[k].float())), f"baseline: {k} does not repeat"
    p = dict(d, input_ids=d["input_ids"].clone())
    cg = int(c[g])
    p["input_ids"][g, 1:cg - 1] = 110 + (d["input_ids"][g, 1:cg - 1] + 271) % 800
    new = gen(p)
    other = [q for q in range(G) if q != g]
    n_out = n_in = 0
    for k in base:
        as_bits = lambda x: bits(x.float()) if x.is_floating_point() else x.numpy()
        a, bb = as_bits(base[k]), as_bits(new[k])
        assert np.array_equal(a[other], bb[other]), f"{k} of dialogs {[q for q in other if not np.array_equal(a[q], bb[q])]} changed with dialog {g}'s context"
        n_out += a[other].size
        if k in ("step_logp", "logp", "scores"):
            n_in += int((a[g] != bb[g]).sum())
    print(f"\n    generate_answers({kw}): {n_out} values of the other dialogs bit-identical, {n_in} log-probabilities of dialog {g} changed")
    assert n_out >= MIN_OUT and n_in >= MIN_IN


# ---------------------------------------------------------------------------------------------------------------------
# 7 dead positions
# ---------------------------------------------------------------------------------------------------------------------
def dis_batch(model, seed=23):
    """discriminative sequences, sequence 2 longer than all the others"""
    from unimm_amd import synth
    rng = np.random.default_rng(seed)
    lens = [[5, 4, 3], [8, 6, 2], [20, 19, 14], [3, 3], [10, 9, 5], [6, 6, 6, 2]]
    rows = [synth.build_sequence(u, "dis", False, T=T, vocab=1000, mask_prob=0.3, rng=rng, start_segment=int(rng.integers(0, 2))) for u in lens]
    B = len(rows)
    stack = lambda k: torch.from_numpy(np.stack([r[k] for r in rows]))
    tgt = rng.random((B, NREG, 101)).astype(np.float32)
    label = np.where(rng.random((B, NREG)) < 0.2, 1, -1)
    label[:, 0] = 0
    b = dict(input_ids=stack("tokens"), token_type_ids=stack("segments"), position_ids=stack("positions"), masked_lm_labels=stack("labels"),
             lm_weight=stack("weights"), attention_mask=stack("txt_attention_mask"),
             co_attention_mask=stack("co_attention_mask")[:, None, :].expand(B, NREG, T).bool().contiguous(),
             image_attention_mask=torch.ones(B, NREG),
             image_feat=torch.from_numpy(np.maximum(rng.standard_normal((B, NREG, 192)), 0).astype(np.float32)),
             image_loc=torch.from_numpy(rng.random((B, NREG, 5)).astype(np.float32)),
             image_target=torch.from_numpy(tgt / tgt.sum(-1, keepdims=True)), image_label=torch.from_numpy(label.astype(np.int64)),
             next_sentence_label=torch.zeros(B, dtype=torch.int64), nsp_weight=torch.tensor([[1.0, 1.0]]))
    assert all(int((b["masked_lm_labels"][s] != -1).sum()) >= 1 for s in range(B))
    return {k: v.cuda() for k, v in b.items()}, [r["L"] for r in rows]


def position_row_grads(model, b):
    """one training step from zeroed gradients -> position_embeddings.weight.grad as [B, T, H] (row b * T + t is text row (b, t)'s)"""
    model.train()
    eng = model.engine
    eng.ensure(torch.device("cuda", 0))
    model.set_dropout_seed(99, 0)
    eng.arena.zero_grads()
    B = b["input_ids"].shape[0]
    assert B * T <= model.config.max_position_embeddings
    pos = torch.arange(B * T, device="cuda").view(B, T)
    kw = {k: b.get(k) for k in KEYS if k != "position_ids"}
    res = model.forward_backward(b["input_ids"], b["image_feat"], b["image_loc"], (1.0, 1.0, 1.0), position_ids=pos, **kw)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in res[:4])
    g = model.bert.embeddings.position_embeddings.weight.grad
    return g[:B * T].detach().float().cpu().numpy().reshape(B, T, -1).copy()


def reachable_rows(model, b):
    """[B, T]: the text input rows that some loss-bearing output reads (flow_ref, backwards)"""
    am, im, co = dense_masks_of(b)
    flow = FR.closure(am, im, co, model.config)
    lab, w = b["masked_lm_labels"].cpu().numpy(), b["lm_weight"].cpu().numpy()
    il, nsl = b["image_label"].cpu().numpy(), b["next_sentence_label"].cpu().numpy()
    cw = b["nsp_weight"].reshape(-1).tolist()
    B = lab.shape[0]
    return np.stack([flow.to_text_rows(s, (lab[s] != -1) & (w[s] != 0), il[s] == 1, nsp=cw[int(nsl[s])] != 0) for s in range(B)])


def check_dead(what, g, live):
    zero = ~(g != 0).any(-1)
    bad = zero & live
    assert not bad.any(), f"{what}: rows {np.argwhere(bad)[:12].tolist()} that a loss reads have a zero gradient"
    leak = ~zero & ~live
    assert not leak.any(), f"{what}: rows {np.argwhere(leak)[:12].tolist()} ({int(leak.sum())}) that no loss can reach have a gradient, " \
                           f"largest {float(np.abs(g[leak]).max()):.3e}"
    print(f"    {what}: {int((~live).sum())} position rows exactly zero, {int(live.sum())} nonzero")
    assert int((~live).sum()) >= MIN_OUT and int(live.sum()) >= MIN_IN


@pytest.mark.parametrize("unpad", [True, False], ids=["unpad", "padded"])
@pytest.mark.parametrize("compute", ENGINES)
def test_dead_positions_discriminative(compute, unpad):
    model = build(compute)
    configure(model, unpad=unpad)
    b, Ls = dis_batch(model)
    j = 2
    assert Ls[j] > max(L for s, L in enumerate(Ls) if s != j) + MIN_OUT
    for k in ("masked_lm_labels", "lm_weight", "image_label", "next_sentence_label"):
        b[k] = b[k].clone()
    keep = (b["masked_lm_labels"][j].clone(), b["lm_weight"][j].clone())
    b["masked_lm_labels"][j], b["lm_weight"][j] = -1, 0
    b["image_label"][j] = -1
    b["image_label"][j, 0] = 0
    b["next_sentence_label"][j] = 1
    b["nsp_weight"] = torch.tensor([[1.0, 0.0]])               # class 1 -- sequence j alone -- weighs nothing
    live = reachable_rows(model, b)
    assert not live[j].any() and all(live[s, :Ls[s]].all() and not live[s, Ls[s]:].any() for s in range(len(Ls)) if s != j)
    print()
    g = position_row_grads(model, b)
    check_dead(f"{compute} unpad={unpad} sequence {j} without a loss", g, live)
    b["masked_lm_labels"][j], b["lm_weight"][j] = keep            # ... and with its labels back: every row of j is read
    assert int((keep[1] != 0).sum()) >= 1
    live2 = reachable_rows(model, b)
    assert live2[j, :Ls[j]].all() and int(live2[j].sum()) == Ls[j]
    g = position_row_grads(model, b)
    check_dead(f"{compute} unpad={unpad} sequence {j} labelled", g, live2)


@pytest.mark.parametrize("unpad", [True, False], ids=["unpad", "padded"])
@pytest.mark.parametrize("compute", ENGINES)
def test_dead_positions_generative(compute, unpad):
    model = build(compute)
    configure(model, unpad=unpad)
    b, info = gen_batch()
    B = len(info)
    b["next_sentence_label"] = torch.tensor([0, 1, 0, 1, 1, 0], device="cuda")
    b["nsp_weight"] = torch.tensor([[1.0, 0.0]])               # the NSP term of sequences 1, 3, 4 weighs nothing
    b["image_label"] = b["image_label"].clone()
    for s in (1, 2, 3):                                          # ... and these have no region in the image loss
        b["image_label"][s, 1:] = -1
    live = reachable_rows(model, b)
    for s, (c, L, n) in enumerate(info):
        # what the generative mask means backwards: the copy rows read rows [1, L - 1) and themselves; row 0 is read by the NSP
        # head alone, and the answer's [SEP] row L - 1 through row 0 alone; the regions read the context
        assert live[s, 1:L - 1].all() and live[s, L:L + n].all() and not live[s, L + n:].any()
        assert live[s, 0] == live[s, L - 1] == (s in (0, 2, 5))
    print()
    check_dead(f"{compute} unpad={unpad} generative", position_row_grads(model, b), live)


# ---------------------------------------------------------------------------------------------------------------------
# 8 shared-context training
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["lm_weight", "advantage"])
def test_shared_training_zero_weight_answer(how):
    from tests.test_gpu_shared_training import run as shared_run, sampled
    from unimm_amd.policy import PolicyObjective, spread
    model = build("bf16")
    configure(model)
    d, sb = sampled(4)
    G, N = sb.shape
    spec = sb.attention_mask
    a = next(k for k in range(N, len(spec)) if int(spec.answer[k]) >= 3)      # an answer of a later dialog, three tokens or more
    L, n = int(spec.length[a]), int(spec.answer[a])
    c = L - n
    other = SimpleNamespace(**vars(sb))
    other.input_ids, other.masked_lm_labels = sb.input_ids.clone(), sb.masked_lm_labels.clone()
    ans = 110 + (sb.input_ids[a, c:L] + 91) % 800
    other.input_ids[a, c:L] = ans
    other.masked_lm_labels[a, L:L + n] = ans
    assert bool((sb.masked_lm_labels[a, L:L + n] != -1).all()) and int((sb.masked_lm_labels[a] != -1).sum()) == n

    def inputs(weight):
        if how == "lm_weight":
            w = (sb.masked_lm_labels != -1).long()
            w[a] *= weight
            return dict(lm_weight=w)
        adv = torch.tensor([[1.0, -0.5, 0.75, -1.25], [0.5, 1.5, -1.0, 0.25], [-0.75, 1.0, 0.5, -0.25]])[:G, :N].clone()
        adv.view(-1)[a] *= weight
        return dict(lm_advantage=spread(adv, sb), lm_objective=PolicyObjective(mode="logp"))

    def step(batch, weight):
        (_, lm, _, _, _), grads = shared_run(model, d, batch, True, seed=41, **inputs(weight))
        assert bool(torch.isfinite(lm).all()) and bool(torch.isfinite(grads).all())
        return bits(lm.reshape(1, 1)), grads.view(torch.int32).cpu().numpy(), grads

    l0, g0, f0 = step(sb, 0)
    l0b, g0b, _ = step(sb, 0)
    assert np.array_equal(l0, l0b) and np.array_equal(g0, g0b), "baseline does not repeat"
    l1, g1, f1 = step(other, 0)
    used = np.zeros(g0.shape, bool)
    for _, lo, hi in model.engine.arena.used_ranges():
        used[lo:hi] = True
    differ = np.nonzero(g0 != g1)[0]
    print(f"\n    {how}: zero-weight answer replaced: loss {'identical' if np.array_equal(l0, l1) else 'DIFFERS'}, "
          f"{int(used.sum())} gradient elements compared bit for bit, {len(differ)} differ")
    assert np.array_equal(l0, l1)
    assert len(differ) == 0, (differ[:8].tolist(), f0[differ[:8]].tolist(), f1[differ[:8]].tolist())
    l2, g2, _ = step(sb, 1)
    l3, g3, _ = step(other, 1)
    n_in = int((g2 != g3).sum())
    print(f"    {how}: weight restored: loss {'differs' if not np.array_equal(l2, l3) else 'IDENTICAL'}, {n_in} gradient elements differ")
    assert not np.array_equal(l2, l3) and n_in >= MIN_IN and int(used.sum()) >= MIN_OUT
