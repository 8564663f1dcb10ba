"""tests/flow_ref.py against the float64 oracle (oracle/vilbert_ref.py), small config, T = 64, R = 37: the closure is a checked
reference, not a second opinion.

One batch of four sequences from oracle/masks.py (two generative -- one with a 1-token answer --, two discriminative; two of
them with masked regions).  One input position is perturbed per case (a text row: token, position and type id; a region:
features and box) and the oracle runs again at the same shapes.  Both directions, without a tolerance:

 (a) every output OUTSIDE the closure -- sequence-output rows, LM score rows, image prediction rows, NSP logits, per-sequence
     likelihoods, of every sequence -- is exactly equal in float64;
 (b) every output in the ONE-LAYER closure (what the input reaches through a single block) changes.

Each live case holds at least 8 compared outputs outside and 4 changed ones inside; the counts are printed (pytest -s).  The dead
cases (a padding row, a masked region) reach no valid output at all: that is what the GPU file's padding check relies on."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import masks as M
from oracle import vilbert_ref as R
from tests import flow_ref as FR

T, NREG = 64, 37
MIN_OUT, MIN_IN = 8, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def oracle_batch(seed=3, vocab=1000, feat=192):
    """-> (dict of tensors with the model's keyword names, per-sequence dict(mode, L, n, c))"""
    rng = np.random.default_rng(seed)
    words = lambda n: rng.integers(110, vocab, size=n).tolist()
    specs = [("gen", [5, 4, 3, 3]), ("dis", [6, 5, 2]), ("gen", [7, 3, 1]), ("dis", [20, 20, 10])]
    rows, info = [], []
    for mode, lens in specs:
        utts = [words(n) for n in lens]
        draws = rng.random(sum(lens))
        if mode == "gen":
            e = M.encode_gen(utts, start_segment=int(rng.integers(0, 2)), max_seq_len=T)
        else:
            e = M.encode_dis(utts, start_segment=int(rng.integers(0, 2)), max_seq_len=T, mask_prob=0.3, mask_draws=draws)
        L = 1 + sum(n + 1 for n in lens)
        n = lens[-1] + 1 if mode == "gen" else 0
        rows.append(e)
        info.append(dict(mode=mode, L=L, n=n, c=L - n, valid=L + n))
    cat = lambda k: torch.from_numpy(np.concatenate([r[k] for r in rows]))
    im = torch.ones(len(rows), NREG)
    im[1, 30:] = 0
    im[2, 20:] = 0
    f = np.maximum(rng.standard_normal((len(rows), NREG, feat)), 0)
    loc = rng.random((len(rows), NREG, 5))
    batch = dict(input_ids=cat("tokens"), token_type_ids=cat("segments"), position_ids=cat("positions"),
                 masked_lm_labels=cat("labels"), attention_mask=cat("txt_attention_mask").bool(),
                 co_attention_mask=cat("co_attention_mask").bool()[:, None, :].expand(len(rows), NREG, T).contiguous(),
                 image_attention_mask=im, image_feat=torch.from_numpy(f), image_loc=torch.from_numpy(loc))
    for b, i in enumerate(info):
        assert int((batch["masked_lm_labels"][b] != -1).sum()) >= 2, (b, i)
    return batch, info


def oracle_outputs(sd, ocfg, b):
    """float64 forward -> dict(seq [B, T, H], lm [B, T, V], img [B, R, C], nsp [B, 2], ll [B])"""
    out = R.forward(sd, ocfg, b["input_ids"], b["image_feat"], b["image_loc"], token_type_ids=b["token_type_ids"],
                    position_ids=b["position_ids"], attention_mask=b["attention_mask"].double(),
                    image_attention_mask=b["image_attention_mask"].double(), co_attention_mask=b["co_attention_mask"].double())
    ll = R.sequence_log_likelihood(out["pred_t"], b["masked_lm_labels"])
    return dict(seq=out["seq_out_t"], lm=out["pred_t"], img=out["pred_v"], nsp=out["nsp"], ll=ll)


def perturb(b, kind, s, i):
    """a copy of the batch with text row (s, i) or region (s, i) changed -- shapes and masks are not touched"""
    p = {k: v.clone() for k, v in b.items()}
    if kind == "text":
        p["input_ids"][s, i] = 110 + (int(b["input_ids"][s, i]) + 417) % 800
        p["position_ids"][s, i] = (int(b["position_ids"][s, i]) + 100) % 512
        p["token_type_ids"][s, i] = 1 - int(b["token_type_ids"][s, i])
    else:
        p["image_feat"][s, i] = b["image_feat"][s, i].flip(0) + 0.5
        p["image_loc"][s, i] = 1.0 - b["image_loc"][s, i]
    return p


def reach_sets(flow, kind, s, i, labels):
    """-> dict of boolean arrays over ALL outputs of the batch: seq / lm [B, T], img [B, R], nsp [B], ll [B]"""
    B, Tn, Rn = flow.B, flow.T, flow.R
    r = flow.from_text(s, i) if kind == "text" else flow.from_region(s, i)
    seq, img, nsp, ll = np.zeros((B, Tn), bool), np.zeros((B, Rn), bool), np.zeros(B, bool), np.zeros(B, bool)
    seq[s], img[s], nsp[s] = r["text"], r["regions"], r["nsp"]
    ll[s] = flow.likelihood(r, labels[s] != -1)
    return dict(seq=seq, lm=seq.copy(), img=img, nsp=nsp, ll=ll)


def changed(base, new):
    """which outputs differ at all, per output row: same layout as reach_sets"""
    rows = lambda k: (base[k] != new[k]).reshape(base[k].shape[0], base[k].shape[1], -1).any(-1).numpy()
    return dict(seq=rows("seq"), lm=rows("lm"), img=rows("img"), nsp=(base["nsp"] != new["nsp"]).any(-1).numpy(),
                ll=(base["ll"] != new["ll"]).numpy())


@pytest.fixture(scope="module")
def case():
    with open(os.path.join(GOLDEN, "small_config.json")) as f:
        ocfg = R.make_config(json.load(f))
    sd = {k: v.double() for k, v in R.init_state_dict(ocfg, seed=11).items()}
    b, info = oracle_batch()
    full = FR.closure(b["attention_mask"], b["image_attention_mask"], b["co_attention_mask"], ocfg)
    near = FR.one_layer(b["attention_mask"], b["image_attention_mask"], b["co_attention_mask"], ocfg)
    with torch.no_grad():
        base = oracle_outputs(sd, ocfg, b)
    return dict(ocfg=ocfg, sd=sd, b=b, info=info, full=full, near=near, base=base)


def sites():
    """(name, kind, sequence, index as a function of the sequence's layout, live)"""
    return [
        ("gen context token", "text", 0, lambda i: 3, True),
        ("gen answer token 0", "text", 0, lambda i: i["c"], True),
        ("gen last answer token", "text", 0, lambda i: i["L"] - 2, True),
        ("gen copy row 0", "text", 0, lambda i: i["L"], True),
        ("gen 1-token answer", "text", 2, lambda i: i["c"], True),
        ("gen first region", "region", 0, lambda i: 0, True),
        ("gen region 17", "region", 0, lambda i: 17, True),
        ("dis first token", "text", 1, lambda i: 0, True),
        ("dis last token", "text", 1, lambda i: i["L"] - 1, True),
        ("dis long sequence, middle", "text", 3, lambda i: 30, True),
        ("dis region beside masked ones", "region", 1, lambda i: 29, True),
        ("gen unmasked region, others masked", "region", 2, lambda i: 5, True),
        ("dis padding row", "text", 1, lambda i: i["L"] + 2, False),
        ("gen padding row", "text", 0, lambda i: i["valid"], False),
        ("masked region", "region", 2, lambda i: 25, False),
    ]


@pytest.mark.parametrize("name,kind,s,where,live", sites(), ids=[x[0].replace(" ", "_").replace(",", "") for x in sites()])
def test_oracle_honours_the_closure(case, name, kind, s, where, live):
    b, info = case["b"], case["info"]
    i = where(info[s])
    with torch.no_grad():
        new = oracle_outputs(case["sd"], case["ocfg"], perturb(b, kind, s, i))
    got = changed(case["base"], new)
    labels = b["masked_lm_labels"].numpy()
    full, near = reach_sets(case["full"], kind, s, i, labels), reach_sets(case["near"], kind, s, i, labels)
    n_out = n_in = n_full = 0
    for k in ("seq", "lm", "img", "nsp", "ll"):
        assert not (near[k] & ~full[k]).any(), k
        leak = got[k] & ~full[k]
        assert not leak.any(), f"{name}: {k} outputs outside the closure changed at {np.argwhere(leak).tolist()[:8]}"
        still = near[k] & ~got[k]
        assert not still.any(), f"{name}: {k} outputs of the one-layer closure did not change at {np.argwhere(still).tolist()[:8]}"
        n_out += int((~full[k]).sum())
        n_in += int(near[k].sum())
        n_full += int((full[k] & got[k]).sum())
    # what the input reaches among the outputs anybody reads: the valid rows and the unmasked regions
    valid = np.zeros((len(info), T), bool)
    for q, inf in enumerate(info):
        valid[q, :inf["valid"]] = True
    live_in = int((full["seq"] & valid).sum()) + int((full["img"] & (b["image_attention_mask"].numpy() != 0)).sum())
    print(f"\n{name} ({kind} {s},{i}): closure {sum(int(full[k].sum()) for k in full)} outputs ({n_full} changed), one-layer closure "
          f"{n_in} (all changed), outside {n_out} (all exactly equal in float64)")
    if live:
        assert n_out >= MIN_OUT and n_in >= MIN_IN, (n_out, n_in)
    else:
        # (a padding row has an empty mask row, reads every key and so the other padding rows: those are all it reaches)
        assert live_in == 0 and not full["nsp"].any() and not full["ll"].any(), live_in


def test_no_edge_between_sequences(case):
    full = case["full"].assert_no_cross_sequence()
    B, N = case["full"].B, T + NREG
    assert full.shape == (B * N, B * N) and full.any()
    # and the closure is not trivially everything inside a sequence: a generative context row never reads the answer
    i = case["info"][0]
    assert not case["full"].tt[0, 1:i["c"], i["c"]:i["L"]].any()
    assert case["full"].tt[0, i["L"] + 1, i["c"]] and not case["full"].tt[0, i["L"], i["c"]]
    # nor the image stream: regions read the context only (co-attention mask), never the answer
    assert not case["full"].vt[0, :, i["c"]:].any() and case["full"].vt[0, :, 1:i["c"]].all()


def test_valid_lengths_match_the_layout(case):
    b, info = case["b"], case["info"]
    got = FR.valid_lengths(b["attention_mask"], b["co_attention_mask"], b["masked_lm_labels"])
    assert got.tolist() == [i["valid"] for i in info]
