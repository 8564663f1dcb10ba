"""The regime case -- TEST INFRASTRUCTURE shared by tests/test_engine_regimes_cpu.py and tests/test_gpu_engine_regimes.py.

The small goldens (hidden 128, intermediate 256, ~150 text rows) take ONE branch of every launch rule of unimm_amd/engine.py:
every GEMM is one column tile wide, no reduction reaches K = 2048, no weight gradient is split.  This module synthesizes one
configuration and one batch at which each rule takes each of its branches, and restates the rules in plain functions that never
call the engine, so that a GPU test can hold a record of what the engine launched against them:

  configuration  tests/golden/small_config.json with intermediate_size = 2048: the text side's FF1 has N = 2048 (128x128 tiles:
                 256 and more from 1,921 rows on), FF2 has K = 2048, N = 128 (the split-K shape); hidden 128, two heads of 64,
                 v_hidden / bi_hidden 256 stay.
  batch          unimm_amd.synth.make_batch, 56 sequences of T = 48, 37 regions, 6 sequences per image, seeded state dict of
                 oracle.vilbert_ref.init_state_dict.  `build()` asserts what the case rests on: 2048 <= valid text rows < B T
                 (real padding), B x 37 >= 2048 image rows, a sequence at most 3/4 as long as the longest and lengths that are
                 not already longest-first (the attention launches' `order` is then not the identity).
  rules          `expected_gemm`: Engine._tile / Engine._splitk as their docstrings and DESIGN.md ("small-batch tile rule",
                 "split-K of long reductions") state them; `expected_overwrite`; `wgrad_calls`: the grouped weight-gradient
                 launches of the step from unimm_amd.bucket_plan (the ledger both the engine and the exchange planner drive),
                 whose launcher-side rules are oracle/gemm_tn_ref.py's (`is_big`, `splits`, `uses_ws`, `ws_bytes`).
  gate           tests/golden/dropout_sentinels_regimes.json: `grad_ref.sentinel_table` (kind "key") over the 33 dropout sites
                 of THIS case; G' = half the smallest sentinel change in it (`gate()`).

Regenerating the table (34 float64 oracle runs of about two seconds each on a CPU):

    python -c "from tests import regime_case; regime_case.write_table()"
"""
import json
import os

import numpy as np

from oracle import gemm_tn_ref as TN
from oracle import vilbert_ref as R
from tests import grad_ref as GR
from unimm_amd import bucket_plan as BP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABLE = os.path.join(GOLDEN, "dropout_sentinels_regimes.json")
SWITCHES = dict(intermediate_size=2048)
N_SEQ, T, REGIONS, PER_IMAGE, BATCH_SEED = 56, 48, 37, 6, 1234
SEED, STEP0 = 77, 4                      # as tests/test_gpu_train_grads.py: forward() bumps the step, the masks are those of step 5
STEP = STEP0 + 1

# ---- the engine's schedule options as this module restates them (tests/test_engine_regimes_cpu.py holds them against a fresh Engine)
DEFAULTS = dict(gemm_tile=0, tile_table={}, small_rows=12000, image_tile=0, splitk=True, unpad=True, lazy_ln=True,
                attn_longest_first=True, wgrad_overwrite=True, wgrad_ws_bytes=0, wgrad_group_rounds=4, skinny_dx_rows=3072,
                row_bucket=1, lm_bucket=1, prune_last_text=True)
IMAGE_TILE_256 = 8                       # bench.py --image-tile: "the 256x256 ping-pong tile" = cfg 8 of unimm_gemm_nt_args.tile
# Tile configurations of include/unimm_hip.h that hold a CU alone: the eight-wave tiles (256x256: 3 lock-step, 8 ping-pong;
# 192x256: 6, and 12 with the X operand on a three-slot ring; 112-128 KiB of LDS) and 10, the 128x128 tile with a three-slot ring
# ("1 per CU").  The four-wave ring tiles 1, 7, 14 are the ones the small-batch rule itself chooses.
ONE_PER_CU_TILES = (3, 6, 8, 10, 12)
TILE_TABLE = {("t", 2048, 128): 7, ("i", 256, 256): 1}

# ---- options outside Engine.schedule_key(), with the reason each may stay outside
OUTSIDE_KEY = {
    "row_bucket": "a capacity: it changes launch SIZES, and the graph executor keys every captured entry on the step's bucketed "
                  "row counts (its signature) beside the schedule key",
    "lm_bucket": "as row_bucket, for the decoded rows",
    "debug_fresh": "a host-side check with a sync of its own; it launches nothing a capture could freeze",
    "host_staging": "how CPU inputs reach the device before the step; the captured launch sequence starts from device tensors",
}


def config_dict():
    with open(os.path.join(GOLDEN, "small_config.json")) as f:
        return dict(json.load(f), **SWITCHES)


def kwargs_of(b):
    """A synth.make_batch dict -> (args, kw) of the model's and the oracle's forward."""
    kw = dict(token_type_ids=b["token_type_ids"], position_ids=b["token_position_ids"], attention_mask=b["attention_mask"],
              image_attention_mask=b["image_attention_mask"], co_attention_mask=b["co_attention_mask"],
              masked_lm_labels=b["masked_lm_labels"], image_label=b["image_label"], image_target=b["image_target"],
              next_sentence_label=b["next_sentence_label"], nsp_weight=b["nsp_weight"], lm_weight=b["lm_weight"])
    return (b["input_ids"], b["image_feat"], b["image_loc"]), kw


_CASE = {}


def build():
    """The case, built once per process -> dict(cfgd, ocfg, sd, args, kw, rows, lens, Mv, Mpad, Mi, n_lm, Mc)."""
    if _CASE:
        return _CASE
    from unimm_amd import BertConfig, synth
    cfgd = config_dict()
    ocfg = R.make_config(cfgd)
    b = synth.make_batch(n_seq=N_SEQ, T=T, R=REGIONS, cfg=BertConfig.from_dict(cfgd), seed=BATCH_SEED, sequences_per_image=PER_IMAGE)
    args, kw = kwargs_of(b)
    rows = GR.packed_rows(kw["attention_mask"], kw["co_attention_mask"], kw["masked_lm_labels"], kw["lm_weight"])
    lens = np.bincount((rows // T).numpy(), minlength=N_SEQ).tolist()
    Mv, Mpad, Mi = int(rows.numel()), N_SEQ * T, N_SEQ * REGIONS
    # the conditions the case is made for (conditions, not measurements)
    assert 2048 <= Mv < Mpad, (Mv, Mpad)                                # FF1 reaches 256 tiles of 128x128; real padding
    assert Mi >= 2048, Mi                                               # the image side's weight gradients may split
    assert min(lens) <= 0.75 * max(lens), (min(lens), max(lens))        # a sequence much shorter than the longest ...
    assert lens != sorted(lens, reverse=True)                           # ... so `order` (longest first) is not the identity
    assert t128(Mv, 2048) >= 256 and t128(Mpad, 2048) >= 256
    n_lm = int((kw["lm_weight"] != 0).sum())                           # decoded rows (oracle/plan_ref.py: weight != 0)
    assert 0 < n_lm and N_SEQ + n_lm not in (Mv, Mpad)                  # the pruned last layer's row count is no step row count
    _CASE.update(cfgd=cfgd, ocfg=ocfg, sd=R.init_state_dict(ocfg, seed=11), args=args, kw=kw, rows=rows, lens=lens, Mv=Mv, Mpad=Mpad,
                 Mi=Mi, n_lm=n_lm, Mc=N_SEQ + n_lm)
    return _CASE


# ---------------------------------------------------------------------------------------------
# the launch rules, restated
# ---------------------------------------------------------------------------------------------
def t128(M, N):
    return -(-M // 128) * -(-N // 128)


def expected_gemm(side, M, N, K, step_rows, opts):
    """(tile code, splitk) of ONE encoder GEMM out[M, N] = x[M, K] w[N, K]^T launched from side "t" (text) or "i" (image) in a
    step of `step_rows` text rows under the engine options `opts` (missing ones = DEFAULTS).  splitk 0 = not split.

      * a non-zero `gemm_tile` goes to every encoder GEMM, and nothing is split;
      * large-batch regime (step_rows >= small_rows): tile 0, the library's choice -- on the image side `image_tile` when that
        is set; no split-K, no table;
      * small-batch regime: split-K (tile 1, 2 workgroups per tile, a workspace) on the text side's full-row GEMMs (M == step
        rows) with K >= 2048, N <= 1024 and at most 256 tiles of 128x128, unless `splitk` is off; else a `tile_table` entry
        (side, N, K); else 14 on the image side; else 7 below 256 tiles of 128x128 and 1 from there on."""
    o = dict(DEFAULTS, **opts)
    if o["gemm_tile"]:
        return o["gemm_tile"], 0
    if step_rows >= o["small_rows"]:
        return (o["image_tile"] if side == "i" else 0), 0
    if o["splitk"] and side == "t" and M == step_rows and K >= 2048 and N <= 1024 and t128(M, N) <= 256:
        return 1, 2
    code = o["tile_table"].get((side, N, K))
    if code is not None:
        return code, 0
    if side == "i":
        return 14, 0
    return (7 if t128(M, N) < 256 else 1), 0


def encoder_gemms(c, opts):
    """Every (side, M, N, K) an encoder block or head of the case's training step launches as an NT GEMM, forward and input
    gradient, as a set -- what the CPU test walks the rules over.  Mt: the step's text rows under `opts`."""
    cfg = c["ocfg"]
    H, Hv, Hb, I, Iv = cfg.hidden_size, cfg.v_hidden_size, cfg.bi_hidden_size, cfg.intermediate_size, cfg.v_intermediate_size
    lmb = dict(DEFAULTS, **opts)["lm_bucket"]
    Mt, Mi, Mc = step_rows(c, opts), c["Mi"], N_SEQ + -(-c["n_lm"] // lmb) * lmb
    pair = lambda side, M, n, k: {(side, M, n, k), (side, M, k, n)}          # forward [N, K] and its input gradient [K, N]
    out = set()
    for n, k in ((3 * H, H), (H, H), (I, H), (H, I), (3 * Hb, H), (H, Hb)):   # self blocks + the text half of a connection layer
        out |= pair("t", Mt, n, k)
    for n, k in ((H, H), (I, H), (H, I)):                                     # the pruned last layer's row-wise half (not its QKV)
        out |= pair("t", Mc, n, k)
    for n, k in ((3 * Hv, Hv), (Hv, Hv), (Iv, Hv), (Hv, Iv), (3 * Hb, Hv), (Hv, Hb)):
        out |= pair("i", Mi, n, k)
    return out


def step_rows(c, opts):
    """Text rows the step computes (Engine._step_rows): the valid rows rounded up to `row_bucket`, or B T on the padded schedule."""
    o = dict(DEFAULTS, **opts)
    if not o["unpad"]:
        return c["Mpad"]
    return min(-(-c["Mv"] // o["row_bucket"]) * o["row_bucket"], c["Mpad"])


def expected_overwrite(N, K, vocab, opts):
    """unimm_gemm_tn_args.overwrite of one queued weight gradient in a backward into a freshly zeroed arena: every problem that
    is the only contribution to its dw -- all but the tied decoder / word-embedding matrix [vocab, hidden] -- unless
    `wgrad_overwrite` is off."""
    return bool(dict(DEFAULTS, **opts)["wgrad_overwrite"]) and N != vocab


def wgrad_calls(c, opts):
    """The grouped weight-gradient calls of the case's backward, in order, from the ledger (unimm_amd.bucket_plan: the rule the
    engine launches by) -> [(side, [TN.Prob, ...])], side 0 = text, 1 = image.  The decoder's input gradient (`_decoder_dx`, a
    grouped call of its own without a bias) is not a weight gradient and not listed.
    The ledger counts the pruned last text layer with the step's rows (Engine._wgrad: rule_M); its problems have Mc rows."""
    from unimm_amd import BertConfig
    o = dict(DEFAULTS, **opts)
    cfg = BertConfig.from_dict(c["cfgd"])
    Mt = step_rows(c, opts)
    n_dec = -(-c["n_lm"] // o["lm_bucket"]) * o["lm_bucket"]
    Mc = N_SEQ + n_dec
    pruned = "t%d" % max(i for k, i in BP.PM.encoder_schedule(cfg) if k == "t") if o["prune_last_text"] else None
    led = BP.Ledger()
    led.begin()
    q, block, calls = [[], []], [], []
    for e in BP.backward_events(cfg, N_SEQ, Mt, n_dec, regions=REGIONS):
        if e[0] == "w":
            _, side, M, N, K = e
            led.queue(side, M, N, K)
            block.append((side, M, N, K))
            continue
        _, group, on_side, force, force_img = e
        for j, (side, M, N, K) in enumerate(block):   # the problems queued since the last mark are this group's
            # the pruned layer's row-wise half (FF2, FF1, attention output: the first three in backward order) runs on Mc rows; its
            # fused QKV projection on all rows
            sub = side == 0 and group == pruned and j < 3
            # a device row count: the MLM head's and the pruned half's rows are capacities; so are all text rows of an unpadded step
            m_dev = side == 0 and (o["unpad"] or group == "heads" or sub)
            q[side].append(TN.Prob(Mc if sub else M, N, K, m_dev))
        block = []
        sides, _ = led.mark(group, o["wgrad_group_rounds"], on_side, force, force_img, hand_over=False)
        for s in sides:
            if q[s]:
                calls.append((s, q[s]))
            q[s] = []
    assert not block and not q[0] and not q[1]
    return calls


def launches_of(calls, shared=True):
    """[(side, chunk of TN.Prob)] per kernel launch of the calls (TN.launches: classes, chunks of 48, descriptor order)."""
    out = []
    for side, probs in calls:
        for _, order in TN.launches(probs):
            out.append((side, [probs[i] for i in order]))
    return out


def ws_bytes_for(c, opts):
    """The weight-gradient workspace the GPU test sets: what the largest launch of the step needs (gemm_tn_ref.ws_bytes, with the
    chip-sharing hint the engine's two-stream step gives), rounded up to 256 bytes."""
    need = max(TN.ws_bytes(chunk, shared=True) for _, chunk in launches_of(wgrad_calls(c, opts)))
    return -(-need // 256) * 256


# ---------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------
def load_table():
    with open(TABLE) as f:
        return json.load(f)


def gate(table=None):
    """G': half the smallest sentinel change of the committed table of this case."""
    table = table or load_table()
    return 0.5 * min(e["change"] for e in table["key"].values())


def weakest(table, n=1):
    return sorted(table["key"], key=lambda s: table["key"][s]["change"])[:n]


def base_run(c, packed=True, mutate=None):
    """One float64 oracle run of the case with the replayed masks of STEP -> dict(losses, nsp, grads, sites)."""
    fn = GR.replay_drop_fn(SEED, STEP, c["rows"] if packed else None, mutate)
    losses, nsp, grads = GR.oracle_grads(c["sd"], c["ocfg"], c["args"], c["kw"], fn)
    return dict(losses=losses, nsp=nsp, grads=grads, sites=sorted(fn.sites))


def compute_table(sites=None, base=None):
    """grad_ref.sentinel_table (kind "key", packed coordinates) over `sites` (default: all 33) in the JSON's layout."""
    c = build()
    sites = GR.site_names(c["ocfg"]) if sites is None else sites
    key, _ = GR.sentinel_table(c["sd"], c["ocfg"], c["args"], c["kw"], SEED, STEP, c["rows"], sites, kind="key", base=base)
    return dict(case=dict(SWITCHES, n_seq=N_SEQ, T=T, regions=REGIONS, sequences_per_image=PER_IMAGE, batch_seed=BATCH_SEED),
                seed=SEED, step=STEP, dtype="float64",
                key={s: dict(sentinel=v[0], change=v[1], max_norm_change=v[2]) for s, v in key.items()})


def write_table():
    doc = compute_table()
    with open(TABLE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {TABLE}: {len(doc['key'])} sites, G' = {gate(doc):.6f}")
