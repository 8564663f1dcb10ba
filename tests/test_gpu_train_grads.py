"""One TRAINING step (model.train(), dropout on at all 33 sites) of the small config, every parameter gradient compared PER
TENSOR in relative L2 with the float64 oracle that replays the engines' counter-based masks (tests/grad_ref.py).

What the per-kernel dropout tests cannot see and the gradient-norm checks of the older train-mode tests do not see either
(tests/test_grad_ref_cpu.py: a 6 % norm check is blind to a wrong mask at 17 of the 33 sites): that the backward of every site
regenerates its mask with the key, step and row coordinates of its forward; that the rows of the pruned last text layer keep the
masks of the rows they came from; that capacities, padding and the second step of a run move no mask.

Gates (none is taken from what the engines give):
  * losses and NSP scores: |got - want| <= tol + tol |want|, tol 2e-2 (bf16) / 1e-3 (fp32x3), as the older train-mode tests;
  * `grad is None` exactly where the oracle has no gradient; numerically zero tensors (key biases, the unused type rows) bounded;
  * bf16: every live tensor's ||g - g_ref|| / ||g_ref|| <= G, G = half the smallest sentinel change of
    tests/golden/dropout_sentinels.json = 0.1323 (sentinel changes 0.265 .. 0.845; derived from the JSON, `grad_ref.gate()`);
  * fp32x3: every live tensor's relative L2 <= 2e-3 (the per-element gate of test_gpu_x3_model.py);
  * negative control (defaults case): against an oracle whose mask at ONE site is that of the next step -- layer.3.out, inside
    the pruned half, and the site with the smallest sentinel change -- that site's sentinel must EXCEED G on both engines.

The fp32x3 engine refuses fixed_t_layer / with_coattention=False (NotImplementedError, asserted in test_gpu_x3_model.py), so the
`frozen` and `nocoatt` cases run on the bf16 engine only.

Measured worst relative L2 of a live tensor (MI355X; the tests print the per-family table):
  case          bf16       fp32x3         case          bf16       fp32x3
  defaults      1.13e-2    1.40e-5        genneg        1.46e-2    1.36e-5
  all_rows      1.13e-2    1.40e-5        dis           1.29e-2    1.51e-5
  padded        1.12e-2    1.46e-5        sumfeat       4.07e-2    1.81e-5
  capacities    1.13e-2    1.40e-5        frozen        1.65e-2    -
  second_step   1.14e-2    1.42e-5        nocoatt       1.35e-2    -
i.e. bf16 at most 0.31 G (sum fusion: c_layer.0.biattention.query1.bias; elsewhere under 0.12 G), fp32x3 at most 0.01 of its gate.
Negative control, sentinel against the mutated oracle: layer.3.out 0.518 (bf16) / 0.519 (fp32x3), v_layer.1.so 0.270 / 0.269.

That the check bites on the engine itself was tried once by hand on the bf16 engine, defaults case: the backward of ONE site given
the key of step 6 -> layer.3.out: 4 tensors above G, its sentinel at 0.489; v_layer.1.so: 7 tensors, sentinel 0.263; the backward
of the pruned layer.3.out without its row map -> 4 tensors above G, worst 0.465 (unbroken: none, worst 0.011).

Per-tensor exceptions: none (EXCEPTIONS is empty)."""
import pytest
import torch

from oracle import vilbert_ref as R
from tests import grad_ref as GR

pytestmark = pytest.mark.gpu

SEED, STEP0 = 77, 4                              # forward() bumps the step: the first step draws the masks of step 5
LOSS_TOL = {"bf16": 2e-2, "fp32x3": 1e-3}
X3_GATE = 2e-3
# bf16 tensors with a gate of their own: {tensor: (gate, reason)}.  Allowed only where fp32x3 passes its gate on the same case and
# masks; the gate is the measured error x 2; at most 10 % of the live tensors; never a sentinel of the committed table.
EXCEPTIONS = {}

#        id               golden           config switches                                   engine options                 steps
CASES = {
    "defaults":        ("small_mixed",   {},                                                {},                              1),
    "all_rows":        ("small_mixed",   {},                                                dict(prune_last_text=False),     1),
    "padded":          ("small_mixed",   {},                                                dict(unpad=False),               1),
    "capacities":      ("small_mixed",   {},                                                dict(row_bucket=64, lm_bucket=16), 1),
    "second_step":     ("small_mixed",   {},                                                {},                              2),
    "genneg":          ("small_genneg",  {},                                                {},                              1),
    "dis":             ("small_dis",     {},                                                {},                              1),
    "sumfeat":         ("small_sumfeat", dict(fusion_method="sum", predict_feature=True),   {},                              1),
    "frozen":          ("small_frozen",  dict(fixed_t_layer=2),                             {},                              1),
    "nocoatt":         ("small_nocoatt", dict(with_coattention=False),                      {},                              1),
}
BF16_ONLY = ("frozen", "nocoatt")
RUNS = [(c, e) for c in CASES for e in ("bf16", "fp32x3") if not (e == "fp32x3" and c in BF16_ONLY)]


@pytest.fixture(scope="module")
def cache():
    """Models per (engine, config switches) and oracle runs per (golden, switches, step, coordinates, mutation): each built once."""
    return dict(models={}, oracle={}, inputs={})


def _inputs(cache, golden_dir, golden, switches):
    k = (golden, tuple(sorted(switches.items())))
    if k not in cache["inputs"]:
        cache["inputs"][k] = GR.load_case(golden_dir, golden, **switches)
    return k, cache["inputs"][k]


def _model(cache, golden_dir, compute, golden, switches):
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    k = (compute, tuple(sorted(switches.items())))
    if k not in cache["models"]:
        _, (_, sd, _, _, cfgd) = _inputs(cache, golden_dir, golden, switches)
        model = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd), compute_dtype=compute)
        model.load_state_dict(sd, strict=True)
        cache["models"][k] = model.cuda()
    return cache["models"][k]


def _oracle(cache, golden_dir, golden, switches, step, packed, mutate=None):
    ik, (ocfg, sd, args, kw, _) = _inputs(cache, golden_dir, golden, switches)
    k = ik + (step, packed, tuple(sorted((mutate or {}).items())))
    if k not in cache["oracle"]:
        rows = GR.packed_rows(kw["attention_mask"], kw["co_attention_mask"], kw["masked_lm_labels"], kw["lm_weight"])
        fn = GR.replay_drop_fn(SEED, step, rows if packed else None, mutate)
        losses, nsp, grads = GR.oracle_grads(sd, ocfg, args, kw, fn)
        cache["oracle"][k] = dict(losses=losses, nsp=nsp, grads=grads, sites=sorted(fn.sites), rows=rows, ocfg=ocfg)
    return cache["oracle"][k]


def _train_steps(model, args, kw, opts, steps):
    """`steps` training steps from (SEED, STEP0) with the engine options set -> what the LAST one gave, its plan and whether its
    last text layer ran on the loss rows only."""
    eng = model.engine
    was = {k: getattr(eng, k) for k in opts}
    pruned = []
    inner = eng._prune_rows
    eng._prune_rows = lambda *a, **k: (pruned.append(inner(*a, **k)), pruned[-1])[1]
    model.train()
    try:
        for k, v in opts.items():
            setattr(eng, k, v)
        model.set_dropout_seed(SEED, step=STEP0)
        for _ in range(steps):
            model.zero_grad(set_to_none=True)
            lm, img, nsp_l, _, _, nsp = model(*args, **kw, _want_lm_scores=False)
            plan = eng.last_plan
            (lm + img + nsp_l).sum().backward()
            torch.cuda.synchronize()
        assert eng.step == STEP0 + steps
        got = dict(losses=dict(lm_loss=lm.detach().cpu(), img_loss=img.detach().cpu(), nsp_loss=nsp_l.detach().cpu()), nsp=nsp.detach().cpu(),
                   grads={n: (None if p.grad is None else p.grad.detach().cpu().clone()) for n, p in model.named_parameters()})
        if plan is not None:
            plan = dict(Mv=plan["Mv"], rows=plan["rows"].cpu().long(), lens_h=list(plan["lens_h"]))
        return got, plan, bool(pruned) and pruned[-1] is not None
    finally:
        del eng._prune_rows
        for k, v in was.items():
            setattr(eng, k, v)
        model.eval()


def _close(got, want, tol, what):
    err = (got.double() - want.double()).abs()
    ratio = float((err / (tol + tol * want.double().abs())).max())
    print(f"  {what}: max |err| {float(err.max()):.3e}, worst |err| / ({tol:g} + {tol:g} |want|) = {ratio:.3f}")
    assert ratio <= 1.0, (what, float(err.max()), ratio)


def _report(c, what):
    fam = {}
    for n, v in c.items():
        if not v["dead"]:
            f = fam.setdefault(GR.family(n), [0.0, 0.0, 0.0, ""])
            if v["l2"] > f[0]:
                f[3] = n
            f[0], f[1], f[2] = max(f[0], v["l2"]), max(f[1], v["norm_err"]), max(f[2], v["max_err"])
    print(f"  {what}: worst per tensor family   ||err|| / ||g||   norm error   max |err| / max |g|")
    for k, f in sorted(fam.items()):
        print(f"    {k:34s} {f[0]:.3e}   {f[1]:.3e}   {f[2]:.3e}   ({f[3]})")
    worst = max((v["l2"], n) for n, v in c.items() if not v["dead"])
    print(f"  {what}: worst relative L2 of a live tensor {worst[0]:.3e} ({worst[1]})")
    return worst


@pytest.mark.parametrize("case,compute", RUNS, ids=[f"{c}-{e}" for c, e in RUNS])
def test_training_step_gradients_match_the_mask_replaying_oracle(golden_dir, cache, case, compute):
    golden, switches, opts, steps = CASES[case]
    table = GR.load_table()
    G = GR.gate(table)
    _, (ocfg, _, args, kw, _) = _inputs(cache, golden_dir, golden, switches)
    model = _model(cache, golden_dir, compute, golden, switches)
    got, plan, pruned = _train_steps(model, args, kw, opts, steps)
    packed = opts.get("unpad", True)
    want = _oracle(cache, golden_dir, golden, switches, STEP0 + steps, packed)
    print(f"\n{case} / {compute}: step {STEP0 + steps}, {'packed' if packed else 'padded'} coordinates, last text layer "
          f"{'on the loss rows' if pruned else 'on all rows'}")

    # ---- the schedule the case is about really ran, and the replay numbered its rows as the engine did
    n_valid = want["rows"].numel()
    assert 0 < n_valid < args[0].numel()                          # every case has padding rows: packed != padded coordinates
    if packed:
        assert plan is not None and torch.equal(plan["rows"][:n_valid], want["rows"]) and sum(plan["lens_h"]) == n_valid
        if "row_bucket" in opts:
            assert plan["Mv"] % opts["row_bucket"] == 0 and plan["Mv"] > n_valid       # a capacity above the real count
        else:
            assert plan["Mv"] == n_valid
    else:
        assert plan is None
    assert pruned == (compute == "bf16" and opts.get("prune_last_text", True))
    assert want["sites"] == GR.site_names(ocfg)
    if ocfg.with_coattention:
        assert want["sites"] == sorted(table["key"])                # the 33 sites of the committed table

    # ---- losses and scores
    tol = LOSS_TOL[compute]
    for k in ("lm_loss", "img_loss", "nsp_loss"):
        _close(got["losses"][k], want["losses"][k], tol, k)
    _close(got["nsp"], want["nsp"], tol, "nsp scores")

    # ---- gradients
    for n, w in want["grads"].items():
        assert (got["grads"][n] is None) == (w is None), (n, "oracle has no gradient" if w is None else "oracle has a gradient")
    assert set(got["grads"]) - set(want["grads"]) <= {R.TIED[0]}               # (the tied decoder is the word-embedding leaf)
    c = GR.compare(got["grads"], want["grads"])
    worst = _report(c, f"{case} / {compute}")
    top = max(v["want_norm"] for v in c.values())
    dead = [n for n, v in c.items() if v["dead"]]
    for n in dead:
        assert c[n]["norm"] <= GR.DEAD_NORM_BOUND * top, (n, c[n])
    live = {n: v for n, v in c.items() if not v["dead"]}
    assert len(live) >= 100 and len(dead) >= 6, (len(live), len(dead))
    if compute == "fp32x3":
        bad = {n: v["l2"] for n, v in live.items() if v["l2"] > X3_GATE}
    else:
        sentinels = {e["sentinel"] for kind in ("key", "coords") for e in table[kind].values()}
        assert not set(EXCEPTIONS) & sentinels and len(EXCEPTIONS) <= 0.1 * len(live)
        bad = {n: v["l2"] for n, v in live.items() if v["l2"] > (EXCEPTIONS[n][0] if n in EXCEPTIONS else G)}
    assert not bad, (f"gate {X3_GATE if compute == 'fp32x3' else G:.4g}", sorted(bad.items(), key=lambda kv: -kv[1])[:8])

    # ---- negative control: a wrong mask at ONE site of the oracle must show at that site's sentinel
    if case == "defaults":
        weakest = min(table["key"], key=lambda s: table["key"][s]["change"])
        for site in ("bert.encoder.layer.3.out", weakest):
            mut = _oracle(cache, golden_dir, golden, switches, STEP0 + steps, packed, {site: "key"})
            sentinel = table["key"][site]["sentinel"]
            cm = GR.compare(got["grads"], mut["grads"])
            print(f"  control: oracle mutated at {site}: sentinel {sentinel} relative L2 {cm[sentinel]['l2']:.4f} "
                  f"(table {table['key'][site]['change']:.4f}, unmutated {c[sentinel]['l2']:.2e}, G {G:.4f}); tensors above their gate: "
                  f"{sum(v['l2'] > (X3_GATE if compute == 'fp32x3' else G) for v in cm.values() if not v['dead'])}")
            assert cm[sentinel]["l2"] > G, (site, sentinel, cm[sentinel])

