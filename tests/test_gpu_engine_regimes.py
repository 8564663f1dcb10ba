"""The launch rules of unimm_amd/engine.py at the row counts where they switch: ONE training step (model.train(), dropout on at
all 33 sites) of the regime case (tests/regime_case.py: intermediate 2048, 56 sequences, 2468 valid of 2688 text rows, 2072 image
rows) per schedule option, on the bf16 engine.  Each case is held against two yardsticks, neither taken from the engine:

  * the float64 oracle with the engines' masks replayed (tests/grad_ref.py): losses and NSP scores within 2e-2 + 2e-2 |want|, the
    `None` set and the dead tensors exactly as tests/test_gpu_train_grads.py, every live tensor's relative L2 <= G' = half the
    smallest sentinel change of tests/golden/dropout_sentinels_regimes.json (`regime_case.gate()`).  The oracle does not depend on
    the engine options: one run for packed and one for padded coordinates, cached per module;
  * a RECORD of every `lib.gemm_nt` and `lib.gemm_tn_grouped` call of the step (the `record` fixture wraps the two module
    attributes the engine calls through): each NT GEMM's (tile, splitk, workspace) must equal `regime_case.expected_gemm`, every
    GEMM shape of the case must have been launched (a branch that did not run fails the case), and the grouped weight-gradient
    calls must be the ledger's list (`regime_case.wgrad_calls`) with the flags oracle/gemm_tn_ref.py's rules expect.

Cases -> what the record must show beyond that (tests/test_engine_regimes_cpu.py proves on the CPU that the case reaches them):
  defaults         split-K (1, 2, workspace) on every full-row FF2 and FF1 input gradient, with the lazy LayerNorm operands on the
                   forward ones; tile 1 on FF1; tile 7 on the N = 128 GEMMs; 14 on the image side; none on the pruned last layer
  no_splitk        FF2 on tile 7, no workspace anywhere
  large_batch      tile 0 everywhere, no split-K;  image_tile: 8 (256x256 ping-pong) on the image side only
  gemm_tile[c]     c on every encoder GEMM, no split-K (1, 7, 14 and the one-per-CU codes 3, 6, 8, 10, 12)
  tile_table       the table's codes on ("t", 2048, 128) and ("i", 256, 256), the default rule elsewhere
  unordered        no `order` list in the plan; losses and NSP scores BIT-identical to `defaults`
  wgrad_ws         padded, all rows in the last layer: a workspace on both sides' calls, not the same one; `uses_ws` for a launch
                   of each side
  wgrad_ws_pruned  the same with the pruned last layer: its problems carry a device row count and share the text side's one
                   launch, so the whole text side stays on atomics
  wgrad_ws_packed  unpadded: image side through the workspace, text side on atomics (device row counts)
  no_overwrite     no `overwrite` flag in any problem (defaults: on every problem but the tied decoder's)
  rounds_1 / _64   the ledger's launches -- for THIS configuration the same as the default's (25 big tiles in a whole backward,
                   the rule needs 224 to launch early: proven in the CPU test), every bucket reported once.  More launches at 1 and
                   fewer at 64 cannot happen at hidden 128, so the record is held against the ledger's list instead.
  capacities       plan["Mv"] = 2688 above the 2468 valid rows, decoded rows 512 above 495
  eager_ln         no aux_ln in any call;  dense_dx: the decoder's input gradient as one NT GEMM [n, 128] x [1024]

Measured worst relative L2 of a live tensor per case (MI355X; G' = 0.1236; the test prints the per-family table):
  defaults         1.632e-2     wgrad_ws         4.688e-2     capacities       1.632e-2
  no_splitk        1.633e-2     wgrad_ws_pruned  4.688e-2     eager_ln         1.632e-2
  large_batch      1.633e-2     wgrad_ws_packed  1.632e-2     dense_dx         1.632e-2
  image_tile       1.633e-2     no_overwrite     1.632e-2     gemm_tile[1, 7, 14, 3, 6, 8, 10, 12]
  tile_table       1.632e-2     rounds_1         1.632e-2                      1.633e-2 each
  unordered        1.632e-2     rounds_64        1.632e-2
i.e. at most 0.38 G' (the padded schedule: bert.v_pooler.dense.bias; the packed one 0.13 G': bert.t_pooler.dense.bias).  Losses
within 2.3e-5, NSP scores within 1.5e-4 of the oracle in every case.  Per-tensor exceptions: none (EXCEPTIONS is empty).

Negative control (defaults): the oracle given the next step's mask at ONE site -- bert.encoder.layer.0.out, the dropout inside the
split-K FF2 epilogue of a full-row layer, and the weakest site of the table, bert.encoder.v_layer.1.out -- that site's sentinel
must exceed G'.  Measured: layer.0.out 0.4187 (table 0.4271), v_layer.1.out 0.2457 (table 0.2472); unmutated 8.9e-3 / 5.7e-3.

That the check bites on the engine itself was tried once by hand: the split-K branch of `Engine._linear` given another dropout key
(the record cannot see that) -> defaults fails with the worst live tensor at 0.393 and more than eight tensors above G';
no_splitk, which never takes the branch, still passes at 1.633e-2.
"""
import pytest
import torch

from oracle import gemm_tn_ref as TN
from oracle import vilbert_ref as R
from tests import grad_ref as GR
from tests import regime_case as RC

pytestmark = pytest.mark.gpu

LOSS_TOL = 2e-2
# tensors with a gate of their own: {tensor: (gate, reason)} -- the rule of tests/test_gpu_train_grads.py: at most 10 % of the
# live tensors, never a sentinel of the committed table, gate = 2 x the measured error
EXCEPTIONS = {}
CONTROL_SITE = "bert.encoder.layer.0.out"


def _cases():
    c = RC.build()
    ws = RC.ws_bytes_for(c, {})
    cases = {
        "defaults": {},
        "no_splitk": dict(splitk=False),
        "large_batch": dict(small_rows=1),
        "image_tile": dict(small_rows=1, image_tile=RC.IMAGE_TILE_256),
        "tile_table": dict(tile_table=dict(RC.TILE_TABLE)),
        "unordered": dict(attn_longest_first=False),
        "wgrad_ws": dict(unpad=False, prune_last_text=False, wgrad_ws_bytes=ws),
        "wgrad_ws_pruned": dict(unpad=False, wgrad_ws_bytes=ws),
        "wgrad_ws_packed": dict(wgrad_ws_bytes=ws),
        "no_overwrite": dict(wgrad_overwrite=False),
        "rounds_1": dict(wgrad_group_rounds=1),
        "rounds_64": dict(wgrad_group_rounds=64),
        "capacities": dict(row_bucket=1024, lm_bucket=256),
        "eager_ln": dict(lazy_ln=False),
        "dense_dx": dict(skinny_dx_rows=0),
    }
    for code in (1, 7, 14) + RC.ONE_PER_CU_TILES:
        cases[f"gemm_tile[{code}]"] = dict(gemm_tile=code)
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def env():
    """The case on the device, the bf16 model, the oracle runs (per coordinates and mutation) and the steps already run."""
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    c = RC.build()
    model = BertForMultiModalPreTraining(BertConfig.from_dict(c["cfgd"]), compute_dtype="bf16")
    model.load_state_dict(c["sd"], strict=True)
    model = model.cuda()
    dev = lambda v: v.cuda() if torch.is_tensor(v) else v
    args = tuple(dev(a) for a in c["args"])
    kw = {k: (v if k == "nsp_weight" else dev(v)) for k, v in c["kw"].items()}       # (nsp_weight is read on the host)
    return dict(case=c, model=model, args=args, kw=kw, oracle={}, steps={}, table=RC.load_table())


def _oracle(env, packed, mutate=None):
    k = (packed, tuple(sorted((mutate or {}).items())))
    if k not in env["oracle"]:
        env["oracle"][k] = RC.base_run(env["case"], packed, mutate)
    return env["oracle"][k]


@pytest.fixture
def record(monkeypatch, env):
    """Wraps unimm_amd.lib.gemm_nt / gemm_tn_grouped: every call is recorded, then made."""
    from unimm_amd import lib as L
    eng = env["model"].engine
    rec = dict(nt=[], tn=[])
    nt, tn = L.gemm_nt, L.gemm_tn_grouped

    def gemm_nt(x, w, out, *a, **kw):
        assert not a                                           # the engine passes everything else by name
        rec["nt"].append(dict(side="i" if eng._on_side else "t", M=kw["M"] if kw.get("M") is not None else x.shape[0],
                              N=kw["N"] if kw.get("N") is not None else w.shape[0], K=kw["K"] if kw.get("K") is not None else x.shape[1],
                              tile=kw.get("tile", 0), splitk=kw.get("splitk", 0), ws=kw.get("splitk_ws") is not None,
                              ws_ptr=kw["splitk_ws"].data_ptr() if kw.get("splitk_ws") is not None else None,
                              epi=kw.get("epilogue", L.EPI_BIAS), aux_ln=kw.get("aux_ln") is not None,
                              drop_rows=kw.get("drop_rows") is not None, aux_rows=kw.get("aux_rows") is not None,
                              encoder=w is not eng.vemb_w))
        return nt(x, w, out, **kw)

    def gemm_tn_grouped(problems, shared=None, ws=None):
        probs = []
        for dy, x, dw, M, N, K, dbias, *rest in problems:
            probs.append(dict(M=dy.shape[0] if M is None else M, N=dy.shape[1] if N is None else N, K=x.shape[1] if K is None else K,
                              bias=dbias is not None, m_dev=bool(rest) and rest[0] is not None, overwrite=len(rest) > 1 and bool(rest[1])))
        rec["tn"].append(dict(side=int(eng._on_side), probs=probs, shared=shared, ws=ws is not None,
                              ws_bytes=ws.numel() if ws is not None else 0, ws_ptr=ws.data_ptr() if ws is not None else None))
        return tn(problems, shared=shared, ws=ws)

    monkeypatch.setattr(L, "gemm_nt", gemm_nt)
    monkeypatch.setattr(L, "gemm_tn_grouped", gemm_tn_grouped)
    return rec


def _train_step(env, opts):
    """One training step from (SEED, STEP0) with the engine options set -> (what it gave, its plan, pruned?, buckets reported)."""
    model = env["model"]
    eng = model.engine
    was = {k: getattr(eng, k) for k in opts}
    pruned, buckets = [], []
    prune_inner, bucket_inner = eng._prune_rows, eng._bucket_done
    eng._prune_rows = lambda *a, **k: (pruned.append(prune_inner(*a, **k)), pruned[-1])[1]
    eng._bucket_done = lambda group, *a, **k: (buckets.append(group), bucket_inner(group, *a, **k))[1]
    model.train()
    try:
        for k, v in opts.items():
            assert hasattr(eng, k), k
            setattr(eng, k, v)
        model.set_dropout_seed(RC.SEED, step=RC.STEP0)
        model.zero_grad(set_to_none=True)
        lm, img, nsp_l, _, _, nsp = model(*env["args"], **env["kw"], _want_lm_scores=False)
        plan = eng.last_plan
        (lm + img + nsp_l).sum().backward()
        torch.cuda.synchronize()
        assert eng.step == RC.STEP
        got = dict(losses=dict(lm_loss=lm.detach().cpu(), img_loss=img.detach().cpu(), nsp_loss=nsp_l.detach().cpu()), nsp=nsp.detach().cpu(),
                   grads={n: (None if p.grad is None else p.grad.detach().cpu().clone()) for n, p in model.named_parameters()})
        if plan is not None:
            order = plan["var"][3]
            plan = dict(Mv=plan["Mv"], rows=plan["rows"].cpu().long(), lens_h=list(plan["lens_h"]),
                        order=None if order is None else order.cpu().long())
        return got, plan, bool(pruned) and pruned[-1] is not None, buckets
    finally:
        del eng._prune_rows, eng._bucket_done
        for k, v in was.items():
            setattr(eng, k, v)
        model.eval()


def _close(got, want, what):
    err = (got.double() - want.double()).abs()
    ratio = float((err / (LOSS_TOL + LOSS_TOL * want.double().abs())).max())
    print(f"  {what}: max |err| {float(err.max()):.3e}, worst |err| / ({LOSS_TOL:g} + {LOSS_TOL:g} |want|) = {ratio:.3f}")
    assert ratio <= 1.0, (what, float(err.max()), ratio)


def _check_numbers(env, case, got, want, G):
    """The gates of the module docstring -> GR.compare's result."""
    table = env["table"]
    for k in ("lm_loss", "img_loss", "nsp_loss"):
        _close(got["losses"][k], want["losses"][k], k)
    _close(got["nsp"], want["nsp"], "nsp scores")
    for n, w in want["grads"].items():
        assert (got["grads"][n] is None) == (w is None), (n, "oracle has no gradient" if w is None else "oracle has a gradient")
    assert set(got["grads"]) - set(want["grads"]) <= {R.TIED[0]}
    c = GR.compare(got["grads"], want["grads"])
    fam = {}
    for n, v in c.items():
        if not v["dead"] and v["l2"] > fam.get(GR.family(n), (0.0, ""))[0]:
            fam[GR.family(n)] = (v["l2"], n)
    for k, (l2, n) in sorted(fam.items()):
        print(f"    {k:34s} {l2:.3e}   ({n})")
    worst = max((v["l2"], n) for n, v in c.items() if not v["dead"])
    print(f"  MEASURED {case}: worst relative L2 of a live tensor {worst[0]:.3e} ({worst[1]}); G' = {G:.4f}")
    top = max(v["want_norm"] for v in c.values())
    dead = [n for n, v in c.items() if v["dead"]]
    for n in dead:
        assert c[n]["norm"] <= GR.DEAD_NORM_BOUND * top, (n, c[n])
    live = {n: v for n, v in c.items() if not v["dead"]}
    assert len(live) >= 100 and len(dead) >= 6, (len(live), len(dead))
    sentinels = {e["sentinel"] for e in table["key"].values()}
    assert not set(EXCEPTIONS) & sentinels and len(EXCEPTIONS) <= 0.1 * len(live)
    bad = {n: v["l2"] for n, v in live.items() if v["l2"] > (EXCEPTIONS[n][0] if n in EXCEPTIONS else G)}
    assert not bad, (f"gate {G:.4g}", sorted(bad.items(), key=lambda kv: -kv[1])[:8])
    return c


def _check_nt_record(env, case, opts, rec, Mt, pruned):
    """Every NT GEMM against the restated rule; every shape of the case launched; the case's own branch really taken."""
    from unimm_amd import lib as L
    c = env["case"]
    cfg = c["ocfg"]
    H, I = cfg.hidden_size, cfg.intermediate_size
    enc = [r for r in rec["nt"] if r["encoder"]]
    other = [r for r in rec["nt"] if not r["encoder"]]
    assert len(other) == 1 and (other[0]["tile"], other[0]["splitk"], other[0]["side"]) == (0, 0, "i")     # the image embedding
    for r in enc:
        want = RC.expected_gemm(r["side"], r["M"], r["N"], r["K"], Mt, opts)
        assert (r["tile"], r["splitk"] if r["ws"] else 0) == want and r["ws"] == (want[1] != 0), (r, want)
    seen = {(r["side"], r["M"], r["N"], r["K"]) for r in enc}
    shapes = RC.encoder_gemms(c, opts)
    if not pruned:
        shapes = {g for g in shapes if g[1] in (Mt, c["Mi"])}
    missing = shapes - seen
    assert not missing, sorted(missing)
    used = {}
    for r in enc:
        used.setdefault((r["tile"], r["splitk"] if r["ws"] else 0), []).append(r)
    print(f"  NT GEMMs: {len(enc)} encoder calls; (tile, splitk) -> calls: " + ", ".join(f"{k}: {len(v)}" for k, v in sorted(used.items())))
    assert set(used) == {RC.expected_gemm(*g, Mt, opts) for g in shapes}
    # split-K launches of one stream share one workspace, and never the image side's
    sk = [r for r in enc if r["ws"]]
    assert len({r["ws_ptr"] for r in sk}) <= 1 and all(r["side"] == "t" and r["M"] == Mt for r in sk)
    # rows-to-masks wiring of the pruned layer: its two residual joins name their rows, nothing else does
    mapped = [r for r in enc if r["drop_rows"]]
    assert all(r["epi"] == L.EPI_BIAS_DROP_RESID and r["M"] != Mt for r in mapped) and len(mapped) == (2 if pruned else 0)
    assert sum(r["aux_rows"] for r in enc) == (1 if pruned else 0)
    # text-side full-row FFN blocks of the step: every text layer but the pruned one, and the text half of every connection layer
    blocks = cfg.num_hidden_layers - (1 if pruned else 0) + len(cfg.v_biattention_id)
    ff2 = [r for r in enc if (r["side"], r["M"], r["N"], r["K"]) == ("t", Mt, H, I)]      # FF2 forward + FF1 input gradient
    ff1 = [r for r in enc if (r["side"], r["M"], r["N"], r["K"]) == ("t", Mt, I, H)]      # FF1 forward + FF2 input gradient
    assert len(ff2) == len(ff1) == 2 * blocks, (len(ff2), len(ff1), blocks)
    lazy = dict(RC.DEFAULTS, **opts)["lazy_ln"]
    fwd_ff2 = [r for r in ff2 if r["epi"] == L.EPI_BIAS_DROP_RESID]
    assert len(fwd_ff2) == blocks and all(r["aux_ln"] == lazy for r in fwd_ff2)              # the residual is the lazy mid LayerNorm
    assert any(r["aux_ln"] for r in enc) == lazy
    return enc, ff1, ff2, sk


def _check_tn_record(env, case, opts, rec):
    """The grouped weight-gradient calls against the ledger's list and gemm_tn_ref's rules."""
    c = env["case"]
    o = dict(RC.DEFAULTS, **opts)
    wg = [r for r in rec["tn"] if r["shared"]]                 # (the engine's two-stream step gives the chip-sharing hint)
    dx = [r for r in rec["tn"] if not r["shared"]]             # the decoder's input gradient as a split reduction: no hint, no bias
    assert all(not r["ws"] and not any(p["bias"] or p["m_dev"] or p["overwrite"] for p in r["probs"]) for r in dx)
    want = RC.wgrad_calls(c, opts)
    got = [(r["side"], [TN.Prob(p["M"], p["N"], p["K"], p["m_dev"]) for p in r["probs"]]) for r in wg]
    key = lambda p: tuple(p[:4])
    assert [(s, sorted(map(key, p))) for s, p in got] == [(s, sorted(map(key, p))) for s, p in want], (got, want)
    vocab = c["ocfg"].vocab_size
    for r in wg:
        assert r["ws"] == (o["wgrad_ws_bytes"] > 0) and r["ws_bytes"] == o["wgrad_ws_bytes"], r
        for p in r["probs"]:
            assert p["overwrite"] == RC.expected_overwrite(p["N"], p["K"], vocab, opts), p
    launches = [(r, [r["probs"][i] for i in order], big) for r in wg
                for big, order in TN.launches([TN.Prob(p["M"], p["N"], p["K"], p["m_dev"]) for p in r["probs"]])]
    as_probs = lambda ch: [TN.Prob(p["M"], p["N"], p["K"], p["m_dev"]) for p in ch]
    info = [(r["side"], big, len(ch), TN.splits(as_probs(ch), shared=True),
             TN.uses_ws(as_probs(ch), r["ws_bytes"] if r["ws"] else None, shared=True)) for r, ch, big in launches]
    print(f"  weight gradients: {len(wg)} grouped calls, launches (side, 256x256 class, problems, splits, workspace used): {info}")
    assert any(big for s, big, *_ in info if s == 1) and not any(big for s, big, *_ in info if s == 0)
    assert any(sp > 1 for *_, sp, _ in info)
    return wg, dx, info


@pytest.mark.parametrize("case", list(CASES))
def test_a_training_step_takes_the_expected_launches_and_matches_the_oracle(env, record, case):
    opts = CASES[case]
    c = env["case"]
    cfg = c["ocfg"]
    H, I, Hv = cfg.hidden_size, cfg.intermediate_size, cfg.v_hidden_size
    G = RC.gate(env["table"])
    eng = env["model"].engine
    got, plan, pruned, buckets = _train_step(env, opts)
    env["steps"][case] = got
    packed = opts.get("unpad", True)
    Mt = RC.step_rows(c, opts)
    print(f"\n{case}: {opts}; step rows {Mt}, {'packed' if packed else 'padded'} coordinates, last text layer "
          f"{'on the loss rows' if pruned else 'on all rows'}")

    # ---- the schedule really ran; the replay numbers its rows as the engine did
    n_valid = c["Mv"]
    if packed:
        assert plan is not None and torch.equal(plan["rows"][:n_valid], c["rows"]) and plan["lens_h"] == c["lens"]
        assert plan["Mv"] == Mt and (Mt > n_valid) == ("row_bucket" in opts)
        ordered = opts.get("attn_longest_first", True)
        assert (plan["order"] is not None) == ordered
        if ordered:                                                # longest first, and not the identity on this batch
            o = plan["order"].tolist()
            assert sorted(o) == list(range(RC.N_SEQ)) and o != list(range(RC.N_SEQ))
            assert [c["lens"][i] for i in o] == sorted(c["lens"], reverse=True)
    else:
        assert plan is None
    assert pruned == opts.get("prune_last_text", True)
    assert sorted(buckets) == sorted(g for g, _, _ in eng.arena.buckets), buckets        # every bucket reported exactly once

    # ---- the record
    enc, ff1, ff2, sk = _check_nt_record(env, case, opts, record, Mt, pruned)
    wg, dx, info = _check_tn_record(env, case, opts, record)
    image = [r for r in enc if r["side"] == "i"]
    text = [r for r in enc if r["side"] == "t"]
    n_lm = -(-c["n_lm"] // opts.get("lm_bucket", 1)) * opts.get("lm_bucket", 1)
    dense_dx = [r for r in text if (r["M"], r["N"], r["K"]) == (n_lm, H, -(-cfg.vocab_size // 64) * 64)]
    if case in ("defaults", "unordered", "no_overwrite", "rounds_1", "rounds_64", "capacities", "eager_ln", "dense_dx",
                "wgrad_ws", "wgrad_ws_pruned", "wgrad_ws_packed"):
        assert len(sk) == len(ff2) and all((r["tile"], r["splitk"], r["ws"]) == (1, 2, True) for r in ff2)
        assert all((r["tile"], r["ws"]) == (1, False) for r in ff1)
        assert all(r["tile"] == 14 and not r["ws"] for r in image) and image
        n128 = [r for r in text if r["N"] == H and r["K"] == H]
        assert n128 and all(r["tile"] == 7 for r in n128)
        if pruned:                                                 # the pruned layer: M != step rows -> no split-K, tile 7
            last = [r for r in text if r["M"] == RC.N_SEQ + n_lm and (r["N"], r["K"]) in ((H, I), (I, H))]
            assert len(last) == 4 and all((r["tile"], r["ws"]) == (7, False) for r in last)
    if case == "no_splitk":
        assert not sk and all(r["tile"] == 7 for r in ff2)
    if case == "large_batch":
        assert not sk and {r["tile"] for r in enc} == {0}
    if case == "image_tile":
        assert not sk and {r["tile"] for r in image} == {RC.IMAGE_TILE_256} and {r["tile"] for r in text} == {0}
    if case.startswith("gemm_tile"):
        assert not sk and {r["tile"] for r in enc} == {opts["gemm_tile"]} and not any(r["splitk"] for r in enc)
    if case == "tile_table":
        hit_t = [r for r in text if (r["N"], r["K"]) == (I, H)]
        hit_i = [r for r in image if (r["N"], r["K"]) == (Hv, Hv)]
        assert hit_t and hit_i and {r["tile"] for r in hit_t} == {7} and {r["tile"] for r in hit_i} == {1}
        assert {r["tile"] for r in image if r not in hit_i} == {14} and len(sk) == len(ff2)
    if case == "eager_ln":
        assert not any(r["aux_ln"] for r in record["nt"])
    if case == "dense_dx":
        assert len(dense_dx) == 1 and not dx
    else:
        assert not dense_dx and len(dx) == 1
    ws_used = {side: [u for s, _, _, _, u in info if s == side] for side in (0, 1)}
    if case == "wgrad_ws":
        assert any(ws_used[0]) and any(ws_used[1])
        assert len({r["ws_ptr"] for r in wg if r["side"] == 0}) == 1 and len({r["ws_ptr"] for r in wg if r["side"] == 1}) == 1
        assert {r["ws_ptr"] for r in wg if r["side"] == 0}.isdisjoint({r["ws_ptr"] for r in wg if r["side"] == 1})
    elif case in ("wgrad_ws_packed", "wgrad_ws_pruned"):
        assert any(ws_used[1]) and not any(ws_used[0])
        assert {r["ws_ptr"] for r in wg if r["side"] == 0}.isdisjoint({r["ws_ptr"] for r in wg if r["side"] == 1})
        if case == "wgrad_ws_packed":
            assert all(p["m_dev"] for r in wg if r["side"] == 0 for p in r["probs"])
    else:
        assert not any(ws_used[0]) and not any(ws_used[1])
    if case == "no_overwrite":
        assert not any(p["overwrite"] for r in record["tn"] for p in r["probs"])
    else:
        assert sum(p["overwrite"] for r in wg for p in r["probs"]) == sum(len(r["probs"]) for r in wg) - 1      # all but the tied decoder
    if case == "capacities":
        assert plan["Mv"] > n_valid and n_lm > c["n_lm"]

    # ---- the numbers
    want = _oracle(env, packed)
    assert want["sites"] == GR.site_names(cfg) == sorted(env["table"]["key"])
    cmp_ = _check_numbers(env, case, got, want, G)
    if case == "unordered":
        if "defaults" not in env["steps"]:
            env["steps"]["defaults"] = _train_step(env, {})[0]
        base = env["steps"]["defaults"]
        for k in ("lm_loss", "img_loss", "nsp_loss"):
            assert torch.equal(got["losses"][k], base["losses"][k]), k
        assert torch.equal(got["nsp"], base["nsp"])

    # ---- negative control: a wrong mask at ONE site of the oracle must show at that site's sentinel
    if case == "defaults":
        table = env["table"]
        for site in (CONTROL_SITE, RC.weakest(table)[0]):
            mut = _oracle(env, packed, {site: "key"})
            sentinel = table["key"][site]["sentinel"]
            cm = GR.compare(got["grads"], mut["grads"])
            print(f"  MEASURED control: oracle mutated at {site}: sentinel {sentinel} relative L2 {cm[sentinel]['l2']:.4f} "
                  f"(table {table['key'][site]['change']:.4f}, unmutated {cmp_[sentinel]['l2']:.2e}, G' {G:.4f}); tensors above the gate: "
                  f"{sum(v['l2'] > G for v in cm.values() if not v['dead'])}")
            assert cm[sentinel]["l2"] > G, (site, sentinel, cm[sentinel])
