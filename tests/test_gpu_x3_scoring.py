"""Shared-context candidate scoring (unimm_amd/scoring.py) on the fp32x3 engine, small config, behind
`sequence_log_likelihood(..., shared_context=<round index>)`.

Three sizes, so that the spliced text self-attention launch reaches the 4-, 8- and 16-tile instantiations of the fp32 attention
kernel with real generative masks: 3 rounds x 6 candidates at T = 64 / 128 / 256.  Every sequence is compared with the CPU oracle
(fp32, one sequence at a time) and with the per-candidate fp32x3 path at the fp32 class tolerance |err| <= 1e-3 + 1e-3 |want|
(tests/test_gpu_x3_model.py); ranks, `average`, mask descriptors, host inputs, the NaN poisoning of a context that is not shared
and the refusals are those of the bf16 path (tests/test_gpu_fullsize.py)."""
import json
import os

import pytest
import torch

from tests.test_gpu_x3_model import build_small, close

pytestmark = pytest.mark.gpu
SIZES = {64: (10, 30), 128: (40, 90), 256: (130, 200)}     # T -> c_range


@pytest.fixture(scope="module")
def small(golden_dir):
    model, ocfg, sd = build_small(golden_dir)
    return model.eval(), ocfg, sd


def make(model, T, device="cuda", a_range=(1, 14)):
    from unimm_amd import synth
    b = synth.make_scoring_batch(rounds=3, options=6, T=T, cfg=model.config, seed=7, a_range=a_range, c_range=SIZES[T], device=device)
    spec = b.pop("mask_spec")
    args = (b["input_ids"], b["image_feat"], b["image_loc"], b["masked_lm_labels"])
    kw = dict(token_type_ids=b["token_type_ids"], position_ids=b["token_position_ids"], attention_mask=b["attention_mask"],
              co_attention_mask=b["co_attention_mask"], image_attention_mask=b["image_attention_mask"])
    return b, spec, args, kw


def oracle_scores(ocfg, sd, b):
    """(scores [B], nsp [B, 2]) of the CPU oracle, one sequence at a time"""
    from oracle import vilbert_ref as R
    sc, nsp = [], []
    c = {k: v.cpu() for k, v in b.items()}
    for i in range(c["input_ids"].shape[0]):
        s = slice(i, i + 1)
        with torch.no_grad():
            o = R.forward(dict(sd), ocfg, c["input_ids"][s], c["image_feat"][s], c["image_loc"][s], token_type_ids=c["token_type_ids"][s],
                          position_ids=c["token_position_ids"][s], attention_mask=c["attention_mask"][s],
                          co_attention_mask=c["co_attention_mask"][s], image_attention_mask=c["image_attention_mask"][s])
            nll = torch.nn.functional.cross_entropy(o["pred_t"].view(-1, o["pred_t"].shape[-1]), c["masked_lm_labels"][s].view(-1),
                                                    ignore_index=-1, reduction="none")
        sc.append(-nll.sum())
        nsp.append(o["nsp"].view(-1)[:2])
    return torch.stack(sc), torch.stack(nsp)


@pytest.mark.parametrize("T", sorted(SIZES))
def test_shared_context_scoring_fp32x3(small, T):
    from unimm_amd.harness import scores_to_ranks
    from unimm_amd.inputs import DialogMaskSpec
    from unimm_amd.scoring import forward_shared
    model, ocfg, sd = small
    b, spec, args, kw = make(model, T)
    B = args[0].shape[0]
    grp = b["context_group"]
    n = torch.as_tensor(spec.answer)
    assert B == 18 and int(n.max()) <= 15 and int((torch.as_tensor(spec.length) + n).max()) <= T
    print()
    # the path is taken: the shared pass itself runs on this engine
    eng = model._engine
    eng.ensure(torch.device("cuda", 0))
    inp = dict(input_ids=args[0], image_feat=args[1], image_loc=args[2], masked_lm_labels=args[3], **kw)
    out = forward_shared(eng, inp, grp)
    assert eng.compute_dtype == "fp32x3" and out["plan"].G == 3 and out["rownll"].shape[0] == int(n.sum()) and bool(out["ok"].all())
    rownll = out["rownll"].clone()
    got, nsp = model.sequence_log_likelihood(*args, shared_context=grp, **kw)
    base, nsp0 = model.sequence_log_likelihood(*args, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and (got < 0).all()
    # the oracle, all 18 sequences
    want, want_nsp = oracle_scores(ocfg, sd, b)
    close(got, want, what=f"T={T} shared scores vs oracle")
    close(nsp, want_nsp, what=f"T={T} shared NSP logits vs oracle")
    # shared vs per-candidate, the same engine
    close(got, base.cpu(), what=f"T={T} shared vs per-candidate scores")
    close(nsp, nsp0.cpu(), what=f"T={T} shared vs per-candidate NSP logits")
    print(f"  T={T} shared vs per-candidate: max |d score| {float((got - base).abs().max()):.3e} on scale {float(base.abs().max()):.3g}, "
          f"max |d nsp| {float((nsp - nsp0).abs().max()):.3e}")
    # ranks inside every round: every pair the oracle separates by more than twice the tolerance keeps its order
    same = same_b = 0
    for r0 in range(0, B, 6):
        w = want[r0:r0 + 6].double()
        rg = scores_to_ranks(got[r0:r0 + 6].cpu().view(1, 1, -1)).view(-1)
        rw = scores_to_ranks(want[r0:r0 + 6].view(1, 1, -1)).view(-1)
        rb = scores_to_ranks(base[r0:r0 + 6].cpu().view(1, 1, -1)).view(-1)
        tol = 1e-3 + 1e-3 * w.abs()                                   # each score may be off by its own tolerance
        far = (w[:, None] - w[None, :]) > tol[:, None] + tol[None, :]
        assert bool((rg[:, None] < rg[None, :])[far].all()), (r0, rg.tolist(), rw.tolist())
        same += int((rg == rw).sum())
        same_b += int((rg == rb).sum())
    print(f"  T={T} ranks identical to the oracle's for {same} of {B} candidates ({100.0 * same / B:.0f} %), "
          f"to the per-candidate schedule's for {same_b} of {B} ({100.0 * same_b / B:.0f} %)")
    # average = sum / n
    avg, _ = model.sequence_log_likelihood(*args, shared_context=grp, average=True, **kw)
    assert float((avg - got / n.to(got)).abs().max()) <= 1e-6 * float(got.abs().max())
    # mask descriptors instead of dense masks: the same packed words; the per-sequence sums are fp32 atomics (order)
    kw2 = dict(kw, attention_mask=DialogMaskSpec(spec.mode, spec.length, spec.answer), co_attention_mask=None)
    got2, _ = model.sequence_log_likelihood(*args, shared_context=grp, **kw2)
    assert float((got - got2).abs().max()) <= 1e-4
    # CPU tensors, as val_lm.py hands them over
    got_h, nsp_h = model.sequence_log_likelihood(*(a.cpu() for a in args), shared_context=grp.cpu(), **{k: v.cpu() for k, v in kw.items()})
    torch.cuda.synchronize()
    assert float((got_h - got).abs().max()) <= 1e-4 and float((nsp_h - nsp).abs().max()) <= 1e-4
    # a context that is not shared is reported, not silently scored against the wrong rows; nothing else changes.  "Nothing" is
    # asserted bit for bit where the arithmetic has a fixed order: the log-likelihoods of the decoded rows.  A score is the sum of
    # its sequence's n <= 15 rows (unimm_segment_sum: in row order since tests/test_gpu_information_flow.py, by one fp32 atomic per
    # row in arrival order when this bound was set): two orders
    # of n terms of one sign differ by less than n 2^-23 |score| (each rounds n - 1 times, by at most 2^-24 of a partial sum <= |score|)
    slack = n.to(got) * 2.0 ** -23 * got.abs()
    def only_nan_at(ids, loc, i):
        o = forward_shared(eng, dict(inp, input_ids=ids, image_loc=loc), grp)
        bad = (~o["ok"]).nonzero().view(-1).tolist()
        rows_equal = torch.equal(o["rownll"], rownll)
        scores = model.sequence_log_likelihood(ids, args[1], loc, args[3], shared_context=grp, **kw)[0]
        keep = torch.ones(B, dtype=torch.bool, device=scores.device)
        keep[i] = False
        d = (scores[keep] - got[keep]).abs()
        print(f"  T={T} sequence {i} poisoned: not ok {bad}, decoded rows bit-equal {rows_equal}, other scores move by at most {float(d.max()):.3e}")
        return bad == [i] and rows_equal and bool(torch.isnan(scores[i])) and int(torch.isnan(scores).sum()) == 1 and bool((d <= slack[keep]).all())
    ids_bad = args[0].clone()
    ids_bad[8, 5] = ids_bad[8, 5] + 1
    assert only_nan_at(ids_bad, args[2], 8)
    loc_bad = args[2].clone()
    loc_bad[13, 7, 2] += 0.25
    assert only_nan_at(args[0], loc_bad, 13)


def test_shared_context_refusals_fp32x3(small, golden_dir):
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    from unimm_amd.scoring import forward_shared
    model, ocfg, sd = small
    b, spec, args, kw = make(model, 128, a_range=(16, 16))          # 1 + 2 x 17 = 35 private rows
    with pytest.raises(ValueError, match="32-row"):
        model.sequence_log_likelihood(*args, shared_context=b["context_group"], **kw)
    b, spec, args, kw = make(model, 128)
    inp = dict(input_ids=args[0], image_feat=args[1], image_loc=args[2], masked_lm_labels=args[3], **kw)
    with pytest.raises(NotImplementedError):                          # the key/value caches are generation's, and generation stays bf16
        forward_shared(model._engine, inp, b["context_group"], cache={})
    cfgd = dict(json.load(open(os.path.join(golden_dir, "small_config.json"))), with_coattention=False)
    m2 = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd), compute_dtype="fp32x3").cuda().eval()
    with pytest.raises(NotImplementedError):
        m2.sequence_log_likelihood(*args, shared_context=b["context_group"], **kw)


def test_shared_context_scoring_bf16_small_config(golden_dir):
    """The same pass on the bf16 engine (it is one definition for both): shared vs per-candidate within 2e-3 of the largest |score|."""
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    from oracle import vilbert_ref as R
    cfgd = json.load(open(os.path.join(golden_dir, "small_config.json")))
    model = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd))
    model.load_state_dict(R.init_state_dict(R.make_config(cfgd), seed=11), strict=True)
    model = model.cuda().eval()
    b, spec, args, kw = make(model, 128)
    got, nsp = model.sequence_log_likelihood(*args, shared_context=b["context_group"], **kw)
    base, nsp0 = model.sequence_log_likelihood(*args, **kw)
    torch.cuda.synchronize()
    scale = float(base.abs().max())
    d, dn = float((got - base).abs().max()), float((nsp - nsp0).abs().max())
    print(f"\nbf16 small config: shared vs per-candidate {d:.3e} ({d / scale:.2e} of scale), NSP logits {dn:.3e}")
    assert torch.isfinite(got).all() and d <= 2e-3 * scale and dn <= 2e-2 * (1 + float(nsp0.abs().max()))
