"""The yardstick of the train-mode gradient tests, checked on the CPU with the project's oracle alone (tests/grad_ref.py,
oracle/vilbert_ref.py in float64; no GPU).

Question: if ONE of the 33 dropout sites of a training step drew a wrong mask -- right keep rate, wrong elements, e.g. a backward
that regenerates its mask with another key, step or row numbering than its forward -- which check would notice?  Measured on
tests/golden/small_mixed.npz, seed 77, step 5, packed rows for the text row-wise sites, each site in turn given the mask of
step 6 (tests/golden/dropout_sentinels.json, recomputed and compared here):

  * a 6 % gradient-NORM check per tensor (what the train-mode tests asserted so far) cannot see 17 of the 33 sites: no tensor's
    norm moves by more than 6 % (largest norm change of those sites 0.9-5.9 %);
  * every site has a SENTINEL, the tensor whose gradient moves most in relative L2, ||g_mut - g|| / ||g||: between 0.265
    (v_layer.1.so -> v_layer.1.attention.self.query.weight) and 0.845 (emb_t -> t_pooler.dense.weight);
  * padded coordinates where packed ones belong ("coords", the 13 text row-wise sites) move their sentinels by 0.295-0.534: all
    above the bar, so they are part of the table;
  * a backward that draws the mask of step 6 where its forward drew that of step 5 ("bwd", reported, not part of the table)
    moves the same sentinels by 0.264-0.640 (the embedding sites move their own LayerNorm / location weights instead), and 19 of
    the 33 such slips are invisible to the 6 % norm check;
  * the oracle in float32 against float64: worst relative L2 of a live tensor 8.3e-7, the floor under every gate.

THE GATE G is half the smallest sentinel change of the committed table: 0.1323.  A per-tensor relative-L2 check at G sees every
site; it is derived from the JSON (`grad_ref.gate()`), here and in the GPU tests, never written as a literal.

`python -m tests.test_grad_ref_cpu` rewrites the JSON from the oracle."""
import json
import os

import pytest
import torch

from tests import grad_ref as GR

ROOT = os.path.dirname(os.path.abspath(__file__))
TABLE = GR.TABLE
CASE, SEED, STEP = "small_mixed", 77, 5
BAR = 0.2                       # every site's sentinel must move at least this much
NORM_GATE = 6e-2                # the norm check of the existing train-mode tests


def rows_of(kw):
    return GR.packed_rows(kw["attention_mask"], kw["co_attention_mask"], kw["masked_lm_labels"], kw["lm_weight"])


def compute(golden_dir):
    """The table of the module docstring, from the oracle: dict in the JSON's layout + what the tests print."""
    ocfg, sd, args, kw, _ = GR.load_case(golden_dir, CASE)
    rows = rows_of(kw)
    sites = GR.site_names(ocfg)
    key, base = GR.sentinel_table(sd, ocfg, args, kw, SEED, STEP, rows, sites, kind="key")
    coords, _ = GR.sentinel_table(sd, ocfg, args, kw, SEED, STEP, rows, [s for s in sites if GR.is_text_rowwise(s)],
                                  kind="coords", base=base)
    entry = lambda v: dict(sentinel=v[0], change=v[1], max_norm_change=v[2])
    doc = dict(case=CASE, seed=SEED, step=STEP, dtype="float64", bar=BAR,
               key={s: entry(v) for s, v in key.items()},
               coords={s: entry(v) for s, v in coords.items() if v[1] >= BAR})
    return doc, dict(ocfg=ocfg, sd=sd, args=args, kw=kw, rows=rows, sites=sites, base=base, coords_all=coords)


@pytest.fixture(scope="module")
def computed(golden_dir):
    torch.manual_seed(0)
    return compute(golden_dir)


def test_committed_sentinel_table_is_what_the_oracle_gives(computed):
    doc, _ = computed
    want = GR.load_table()
    assert {k: want[k] for k in ("case", "seed", "step", "dtype", "bar")} == {k: doc[k] for k in ("case", "seed", "step", "dtype", "bar")}
    for kind in ("key", "coords"):
        assert sorted(want[kind]) == sorted(doc[kind]), kind
        for s, e in want[kind].items():
            got = doc[kind][s]
            assert got["sentinel"] == e["sentinel"], (kind, s, got, e)
            assert abs(got["change"] - e["change"]) <= 1e-6 and abs(got["max_norm_change"] - e["max_norm_change"]) <= 1e-6, (kind, s, got, e)


def test_every_site_has_a_sentinel_above_the_bar_and_most_are_invisible_to_norms(computed):
    doc, extra = computed
    key = doc["key"]
    per = ("attn", "so", "out")
    want_sites = ["emb_t", "emb_v", "fuse"] + [f"bert.encoder.layer.{i}.{s}" for i in range(4) for s in per] \
        + [f"bert.encoder.v_layer.{i}.{s}" for i in range(2) for s in per] \
        + [f"bert.encoder.c_layer.{i}.{s}" for i in range(2) for s in ("attn1", "attn2", "bo1", "bo2", "vout", "tout")]
    assert len(want_sites) == 33 and sorted(key) == sorted(want_sites)
    # ... and they are the sites the forward really visits, each once
    fn = GR.replay_drop_fn(SEED, STEP, extra["rows"])
    GR.oracle_grads(extra["sd"], extra["ocfg"], extra["args"], extra["kw"], fn)
    assert sorted(fn.sites) == sorted(want_sites)
    assert 0 < extra["rows"].numel() < extra["args"][0].numel()             # the case really has padding: packed != padded
    print()
    for s in sorted(key, key=lambda s: key[s]["change"]):
        e = key[s]
        print(f"  {s:34s} -> {e['sentinel']:56s} change {e['change']:.4f}   largest norm change {e['max_norm_change']:.4f}")
    low = {s: e["change"] for s, e in key.items() if e["change"] < BAR}
    assert not low, low
    blind = sorted(s for s, e in key.items() if e["max_norm_change"] <= NORM_GATE)
    changes = [e["change"] for e in key.values()]
    print(f"sentinel changes {min(changes):.4f} .. {max(changes):.4f}; G = {GR.gate(doc):.4f}; a {NORM_GATE:.0%} norm check cannot see "
          f"{len(blind)} of {len(key)} sites")
    assert len(blind) == 17, blind               # (the number of the module docstring; it is why the per-tensor L2 gate exists)
    assert abs(GR.gate(doc) - GR.gate()) <= 1e-6 and 0.1 <= GR.gate() <= 0.5 * max(changes)
    # dead tensors: the ten key biases and the unused half of the type table; never a sentinel
    dead = sorted(n for n, v in GR.compare(extra["base"], extra["base"]).items() if v["dead"])
    assert len(dead) == 11 and all(n.endswith(("key.bias", "key1.bias", "key2.bias", "token_type_embeddings_extension.weight")) for n in dead)
    assert not {e["sentinel"] for e in key.values()} & set(dead)


def test_wrong_row_coordinates_move_the_sentinels_too(computed):
    doc, extra = computed
    allc = extra["coords_all"]
    assert sorted(allc) == sorted(s for s in extra["sites"] if GR.is_text_rowwise(s)) and len(allc) == 13
    print()
    for s, v in sorted(allc.items(), key=lambda kv: kv[1][1]):
        print(f"  coords {s:34s} -> {v[0]:56s} change {v[1]:.4f}   largest norm change {v[2]:.4f}   {'in the table' if v[1] >= BAR else 'report only'}")
    assert sorted(doc["coords"]) == sorted(s for s, v in allc.items() if v[1] >= BAR)


def test_fp32_oracle_against_fp64_is_the_floor(computed):
    _, extra = computed
    g32 = GR.oracle_grads(extra["sd"], extra["ocfg"], extra["args"], extra["kw"], GR.replay_drop_fn(SEED, STEP, extra["rows"]),
                          dtype=torch.float32)[2]
    assert all(v.dtype == torch.float32 for v in g32.values() if v is not None)
    assert all(v.dtype == torch.float64 for v in extra["base"].values() if v is not None)
    c = GR.compare(g32, extra["base"])
    worst = max(v["l2"] for v in c.values() if not v["dead"])
    print(f"\nfp32 oracle vs fp64 oracle, same masks: worst relative L2 of a live tensor {worst:.2e}")
    assert worst <= 1e-4 * GR.gate()                # fp32 rounding (2^-24 per operation) is nowhere near the gate
    assert sorted(n for n, v in g32.items() if v is None) == sorted(n for n, v in extra["base"].items() if v is None)


def test_the_next_step_and_the_other_coordinates_are_other_gradients(computed):
    """What the `second_step` and `padded` cases of tests/test_gpu_train_grads.py rest on: with ALL masks taken from step 6, or all
    text row-wise sites numbered over the padded rows, every sentinel moves by more than 2 G -- an engine whose step counter stood
    still, or that numbered its rows the other way, would be more than G (its own noise allowance) away from the oracle."""
    doc, extra = computed
    G = GR.gate(doc)
    sentinels = {e["sentinel"] for e in doc["key"].values()}
    run = lambda step, rows: GR.oracle_grads(extra["sd"], extra["ocfg"], extra["args"], extra["kw"], GR.replay_drop_fn(SEED, step, rows))[2]
    c = GR.compare(run(STEP + 1, extra["rows"]), extra["base"])
    low = min(c[n]["l2"] for n in sentinels)
    print(f"\nstep {STEP + 1} against step {STEP}: smallest relative L2 change of a sentinel {low:.3f} (2 G = {2 * G:.3f})")
    assert low > 2 * G
    c = GR.compare(run(STEP, None), extra["base"])
    text = {e["sentinel"] for e in doc["coords"].values()}
    low = min(c[n]["l2"] for n in text)
    print(f"padded against packed coordinates: smallest relative L2 change of a text-side sentinel {low:.3f}")
    assert low > 2 * G


def test_a_backward_that_draws_another_mask_than_its_forward_moves_the_same_sentinels(computed):
    """The slip the GPU tests exist for, modelled in the oracle: the forward of ONE site uses the right mask, its backward the
    mask of the next step.  Report per site; every site moves some tensor by at least the bar, and every site but the two
    embedding sites (whose parameters lie upstream of the mask) moves the sentinel of the committed table."""
    doc, extra = computed
    bwd, _ = GR.sentinel_table(extra["sd"], extra["ocfg"], extra["args"], extra["kw"], SEED, STEP, extra["rows"], extra["sites"],
                               kind="bwd", base=extra["base"])
    print()
    for s, v in sorted(bwd.items(), key=lambda kv: kv[1][1]):
        print(f"  bwd {s:34s} -> {v[0]:56s} change {v[1]:.4f}   largest norm change {v[2]:.4f}")
    low = min(v[1] for v in bwd.values())
    blind = sum(v[2] <= NORM_GATE for v in bwd.values())
    print(f"backward-only slips: changes {low:.4f} .. {max(v[1] for v in bwd.values()):.4f}; a {NORM_GATE:.0%} norm check cannot see {blind} of {len(bwd)}")
    assert low >= BAR and blind >= 17
    same = [s for s, v in bwd.items() if v[0] == doc["key"][s]["sentinel"]]
    assert sorted(set(bwd) - set(same)) == ["emb_t", "emb_v"]
    # a gate of G leaves room for the engines' own error: what a slip moves, less G, is still more than the bf16 engine's worst
    # measured error on this config (4.1e-2, tests/test_gpu_train_grads.py)
    assert low - GR.gate(doc) > 0.1


def test_mutations_change_exactly_what_they_name(computed):
    """The replay helper itself: a mutated site differs from the base mask, every other site does not; padded and packed
    coordinates agree on a batch without padding and differ with it."""
    _, extra = computed
    rows = extra["rows"]
    x = torch.ones(6, 64, 128, dtype=torch.float64)
    base, key, co = (GR.replay_drop_fn(SEED, STEP, rows, m) for m in (None, {"emb_t": "key"}, {"emb_t": "coords"}))
    a, b, c = base("emb_t", x, 0.1), key("emb_t", x, 0.1), co("emb_t", x, 0.1)
    assert not torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(c, GR.replay_drop_fn(SEED, STEP, None)("emb_t", x, 0.1))
    assert torch.equal(b, GR.replay_drop_fn(SEED, STEP + 1, rows)("emb_t", x, 0.1))
    assert torch.equal(base("fuse", x[0], 0.1), key("fuse", x[0], 0.1))
    full = torch.arange(6 * 64)
    assert torch.equal(GR.replay_drop_fn(SEED, STEP, full)("emb_t", x, 0.1), GR.replay_drop_fn(SEED, STEP, None)("emb_t", x, 0.1))
    flat = a.view(-1, 128)
    pad = torch.ones(6 * 64, dtype=torch.bool)
    pad[rows] = False
    assert (flat[pad] == 1.0 / 0.9).all()                                    # rows outside the plan are never computed: kept
    keep = (flat[rows] != 0).double().mean()
    assert abs(float(keep) - 0.9) < 0.01 and set(flat[rows].unique().tolist()) <= {0.0, 1.0 / 0.9}
    assert base.sites == ["emb_t", "fuse"]
    with pytest.raises(ValueError):
        GR.replay_drop_fn(SEED, STEP, rows, {"fuse": "coords"})


if __name__ == "__main__":
    doc, _ = compute(os.path.join(ROOT, "golden"))
    with open(TABLE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {TABLE}: {len(doc['key'])} sites, {len(doc['coords'])} coordinate entries, G = {GR.gate(doc):.6f}")
