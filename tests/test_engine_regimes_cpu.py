"""CPU proof of the regime case (tests/regime_case.py; no GPU): the synthesized configuration really drives every launch rule of
unimm_amd/engine.py through every branch that tests/test_gpu_engine_regimes.py names, before a GPU minute is spent on it.

  * the restated NT-GEMM rule (`regime_case.expected_gemm`) over the step's GEMM shapes takes tile 7, tile 1, tile 14, split-K,
    the large-batch 0, a table hit and a table miss -- and split-K is NOT taken on the pruned last layer (M != step rows);
  * oracle/gemm_tn_ref.py over the step's grouped weight-gradient launches (from the ledger of unimm_amd/bucket_plan.py): a
    256x256-class problem on the image side, a 128x128-class one on the text side, a split reduction, the workspace used with the
    size the GPU test sets (from `ws_bytes`, a few MiB, not the production 512 MiB) and not used where a chunk carries a device row
    count;
  * `wgrad_group_rounds`: this configuration queues at most a few dozen 256x256 tiles in a whole backward, far from the 224 the
    ledger's rule needs to send a launch early, so 1, 4 and 64 give the SAME launches here -- asserted, because the GPU cases
    `rounds_1` / `rounds_64` hold the engine's record against exactly this list (that the rule itself makes more / fewer launches
    where tiles abound is tests/test_bucket_plan_cpu.py's subject);
  * `Engine.schedule_key()` moves with every option of the GPU test's table, one at a time, on an engine that never saw a
    device; the options outside the key are listed with their reasons (`regime_case.OUTSIDE_KEY`);
  * the committed sentinel table tests/golden/dropout_sentinels_regimes.json: the base run and the three weakest sites are
    recomputed and compared; G' = half the smallest change."""
import pytest
import torch

from oracle import gemm_tn_ref as TN
from tests import grad_ref as GR
from tests import regime_case as RC


@pytest.fixture(scope="module")
def case():
    return RC.build()


def _engine(case):
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    return BertForMultiModalPreTraining(BertConfig.from_dict(case["cfgd"])).engine


def test_the_case_meets_its_conditions(case):
    c = case
    print(f"\nvalid text rows {c['Mv']} of {c['Mpad']}, image rows {c['Mi']}, decoded rows {c['n_lm']}, pruned layer rows {c['Mc']}, "
          f"lengths {min(c['lens'])} .. {max(c['lens'])}")
    assert 2048 <= c["Mv"] < c["Mpad"] and c["Mi"] >= 2048
    assert min(c["lens"]) <= 0.75 * max(c["lens"]) and c["lens"] != sorted(c["lens"], reverse=True)
    assert c["ocfg"].intermediate_size == 2048 and c["ocfg"].hidden_size == 128 and c["ocfg"].v_hidden_size == 256
    assert GR.site_names(c["ocfg"]) == sorted(RC.load_table()["key"]) and len(RC.load_table()["key"]) == 33


def test_restated_defaults_are_the_engines(case):
    eng = _engine(case)
    for k, v in RC.DEFAULTS.items():
        assert getattr(eng, k) == v, k
    assert eng.arena is None                                    # Engine.__init__ touched no device


def _branches(case, opts):
    Mt = RC.step_rows(case, opts)
    return {g: RC.expected_gemm(*g, Mt, opts) for g in sorted(RC.encoder_gemms(case, opts))}, Mt


def test_the_gemm_rule_takes_every_branch_the_gpu_cases_name(case):
    cfg = case["ocfg"]
    H, I, Hv = cfg.hidden_size, cfg.intermediate_size, cfg.v_hidden_size
    # ---- defaults: 7, 1, 14, split-K; no split-K on the pruned layer
    for opts in ({}, dict(unpad=False)):
        b, Mt = _branches(case, opts)
        assert b[("t", Mt, H, I)] == (1, 2)                     # FF2 forward and FF1's input gradient: K = 2048, N = 128
        assert b[("t", Mt, I, H)] == (1, 0)                     # FF1 forward, FF2's input gradient: 256 tiles of 128x128 and more
        assert b[("t", Mt, 3 * H, H)] == (7, 0) and b[("t", Mt, H, H)] == (7, 0)
        assert b[("t", case["Mc"], H, I)] == (7, 0)             # the pruned last layer: M != step rows
        assert b[("t", case["Mc"], I, H)] == (7, 0)             # ... and fewer than 256 tiles
        assert all(v == (14, 0) for g, v in b.items() if g[0] == "i")
        assert {v for v in b.values()} == {(1, 2), (1, 0), (7, 0), (14, 0)}
    b, Mt = _branches(case, dict(splitk=False))
    assert b[("t", Mt, H, I)] == (7, 0) and (1, 2) not in b.values()
    # ---- large batch
    b, Mt = _branches(case, dict(small_rows=1))
    assert set(b.values()) == {(0, 0)}
    b, Mt = _branches(case, dict(small_rows=1, image_tile=RC.IMAGE_TILE_256))
    assert {v for g, v in b.items() if g[0] == "i"} == {(8, 0)} and {v for g, v in b.items() if g[0] == "t"} == {(0, 0)}
    # (image_tile alone, in the small-batch regime, changes nothing)
    assert _branches(case, dict(image_tile=RC.IMAGE_TILE_256))[0] == _branches(case, {})[0]
    # ---- an explicit code
    for code in (1, 7, 14) + RC.ONE_PER_CU_TILES:
        b, _ = _branches(case, dict(gemm_tile=code))
        assert set(b.values()) == {(code, 0)}
    # ---- the table: a hit on each side, misses elsewhere, split-K untouched
    b, Mt = _branches(case, dict(tile_table=RC.TILE_TABLE))
    d, _ = _branches(case, {})
    assert b[("t", Mt, I, H)] == (7, 0) != d[("t", Mt, I, H)] and b[("i", case["Mi"], Hv, Hv)] == (1, 0) != d[("i", case["Mi"], Hv, Hv)]
    hits = {g for g in b if (g[0], g[2], g[3]) in RC.TILE_TABLE}
    assert hits and all(b[g] == d[g] for g in b if g not in hits) and len(b) > len(hits)
    assert b[("t", Mt, H, I)] == (1, 2)
    # in the large-batch regime the table is not read
    assert set(_branches(case, dict(tile_table=RC.TILE_TABLE, small_rows=1))[0].values()) == {(0, 0)}


def test_the_weight_gradient_rules_take_every_branch(case):
    c = case
    calls = RC.wgrad_calls(c, {})
    launches = RC.launches_of(calls)
    assert sorted({s for s, _ in calls}) == [0, 1]
    big = lambda ch: TN.is_big(ch[0].M, ch[0].N, ch[0].K)
    assert any(big(ch) for s, ch in launches if s == 1)                          # 256x256 class: image side (N, K >= 256)
    assert not any(big(ch) for s, ch in launches if s == 0)                      # hidden 128: the text side stays on 128x128
    assert any(TN.splits(ch, shared=True) > 1 for _, ch in launches)
    assert all(p.m_dev for s, ch in launches if s == 0 for p in ch)              # unpadded: every text-side problem has a device count
    # ---- the workspace the GPU test sets
    ws = RC.ws_bytes_for(c, dict(unpad=False, prune_last_text=False))
    assert ws == RC.ws_bytes_for(c, {}) and TN.COUNTER_BYTES < ws < 64 << 20, ws
    print(f"\nweight-gradient workspace of the case: {ws} bytes ({ws / 2**20:.1f} MiB)")
    for opts, text_ws in ((dict(unpad=False, prune_last_text=False), True), (dict(unpad=False), False), ({}, False)):
        L = RC.launches_of(RC.wgrad_calls(c, opts))
        used = {side: [TN.uses_ws(ch, ws, shared=True) for s, ch in L if s == side] for side in (0, 1)}
        assert any(used[1]), opts                                                # image side: through the workspace
        assert any(used[0]) == text_ws, (opts, used)
        assert not any(TN.uses_ws(ch, None, shared=True) for _, ch in L)         # no workspace, no slabs
        for s, ch in L:
            if any(p.m_dev for p in ch):
                assert not TN.uses_ws(ch, ws, shared=True)                       # a device row count in the chunk: atomics
    # the padded step with pruning: ONE text launch holds the pruned layer's problems (a device count) -> the whole chunk on atomics
    L = RC.launches_of(RC.wgrad_calls(c, dict(unpad=False)))
    text = [ch for s, ch in L if s == 0]
    assert any(any(p.m_dev for p in ch) and not all(p.m_dev for p in ch) for ch in text)
    # ---- capacities: a text-side split may own no real rows (the launch is sized for Mv = 2688, 2468 are real)
    Mt = RC.step_rows(c, dict(row_bucket=1024, lm_bucket=256))
    assert Mt > c["Mv"]
    ch = [ch for s, ch in RC.launches_of(RC.wgrad_calls(c, dict(row_bucket=1024, lm_bucket=256))) if s == 0 and ch[0].M == Mt][0]
    s = TN.splits(ch, shared=True)
    assert s > 1 and TN.rows_per_split(Mt, s) * (s - 1) < c["Mv"] < Mt           # (here the last split is short, not empty)
    dec = [ch for s_, ch in RC.launches_of(RC.wgrad_calls(c, dict(row_bucket=1024, lm_bucket=256))) if s_ == 0 and ch[0].M != Mt][0]
    assert dec[0].M == -(-c["n_lm"] // 256) * 256 > c["n_lm"]                    # decoded rows: a capacity above the real count


def test_group_rounds_do_not_move_this_cases_launches(case):
    shape = lambda calls: [(s, [tuple(p) for p in probs]) for s, probs in calls]
    base = shape(RC.wgrad_calls(case, {}))
    tiles = sum(RC.BP.big_tiles_of(p.M, p.N, p.K) for _, probs in RC.wgrad_calls(case, {}) for p in probs)
    print(f"\n256x256 tiles queued over the whole backward: {tiles}; grouped calls {[(s, len(p)) for s, p in base]}")
    assert tiles < RC.BP.CHIP_SLOTS - 32 and max(len(p) for _, p in base) < 40          # neither flush rule can fire early
    for r in (1, 64):
        assert shape(RC.wgrad_calls(case, dict(wgrad_group_rounds=r))) == base


# option -> a value other than its default; the GPU test's table, one entry per option it sets
KEY_OPTIONS = dict(splitk=False, small_rows=1, image_tile=RC.IMAGE_TILE_256, gemm_tile=7, tile_table=RC.TILE_TABLE, attn_longest_first=False,
                   unpad=False, wgrad_ws_bytes=1 << 20, wgrad_overwrite=False, wgrad_group_rounds=1, lazy_ln=False, skinny_dx_rows=0,
                   prune_last_text=False)


def test_schedule_key_moves_with_every_option_of_the_table(case):
    eng = _engine(case)
    base = eng.schedule_key()
    assert eng.schedule_key() == base
    for k, v in KEY_OPTIONS.items():
        was = getattr(eng, k)
        assert was != v, k
        setattr(eng, k, v)
        assert eng.schedule_key() != base, k
        setattr(eng, k, was)
        assert eng.schedule_key() == base, k
    eng.wgrad_group_rounds = 64
    assert eng.schedule_key() != base
    eng.wgrad_group_rounds = 4
    # deliberately outside the key, each with its reason
    assert sorted(RC.OUTSIDE_KEY) == ["debug_fresh", "host_staging", "lm_bucket", "row_bucket"]
    for k, why in RC.OUTSIDE_KEY.items():
        was = getattr(eng, k)
        setattr(eng, k, 256 if isinstance(was, int) and not isinstance(was, bool) else not was)
        assert eng.schedule_key() == base and len(why) > 20, k
        setattr(eng, k, was)
    assert eng.arena is None


def test_committed_sentinel_table_is_what_the_oracle_gives(case):
    table = RC.load_table()
    assert table["seed"] == RC.SEED and table["step"] == RC.STEP and table["dtype"] == "float64"
    assert table["case"] == dict(RC.SWITCHES, n_seq=RC.N_SEQ, T=RC.T, regions=RC.REGIONS, sequences_per_image=RC.PER_IMAGE,
                                 batch_seed=RC.BATCH_SEED)
    base = RC.base_run(case)
    assert base["sites"] == sorted(table["key"])
    weak = RC.weakest(table, 3)
    got = RC.compute_table(sites=weak, base=base["grads"])["key"]
    print()
    for s in weak:
        e = table["key"][s]
        print(f"  {s:34s} -> {e['sentinel']:56s} change {e['change']:.4f} (recomputed {got[s]['change']:.4f})")
        assert got[s]["sentinel"] == e["sentinel"]
        assert abs(got[s]["change"] - e["change"]) <= 1e-6 and abs(got[s]["max_norm_change"] - e["max_norm_change"]) <= 1e-6
    changes = [e["change"] for e in table["key"].values()]
    G = RC.gate(table)
    print(f"sentinel changes {min(changes):.4f} .. {max(changes):.4f}; G' = {G:.4f}")
    assert G == 0.5 * min(changes) == 0.5 * table["key"][weak[0]]["change"] and 0.1 <= G
    # the site of the GPU test's first negative control lies inside a split-K FF2 epilogue on a full-row layer
    assert table["key"]["bert.encoder.layer.0.out"]["change"] > 2 * G
    # dead tensors are never sentinels; live / dead counts as the GPU test expects them
    cmp_ = GR.compare(base["grads"], base["grads"])
    dead = {n for n, v in cmp_.items() if v["dead"]}
    assert not {e["sentinel"] for e in table["key"].values()} & dead
    assert len(cmp_) - len(dead) >= 100 and len(dead) >= 6
    assert all(torch.isfinite(v).all() for v in base["losses"].values())
