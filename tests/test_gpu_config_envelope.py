"""Both engines on the four configurations of tests/envelope_case.py: head sizes, head counts and widths that
`BertConfig.validate_for_hip()` admits and no other model-level test runs (text heads of 128, image / connection heads of 64,
Hb != Hv, Hv < H, 1 / 3 / 5 / 7 heads, widths that are odd multiples of 64, a connection before the first text layer).  The
kernel edge suites cover these shapes one kernel at a time; this is the engine wiring: views, leading dimensions, head counts
handed to launches, mask coordinates, arena layout.

(a) One TRAINING step per (config, engine), the body of tests/test_gpu_train_grads.py: losses and NSP scores at LOSS_TOL,
    `grad is None` where the oracle has none, dead tensors bounded, every live tensor's relative L2 against the float64
    mask-replaying oracle <= 2e-3 (fp32x3) / <= G = 0.1323 (bf16; that G sees a wrong mask at each of the 96 sites of these
    configurations is asserted in tests/test_config_envelope_cpu.py), the EXCEPTIONS rule of that file unchanged (none needed).
    Negative control: against the oracle mutated at two sites (the last text layer's output dropout, a text row-wise site, and
    the last connection layer's image-side output dropout) some live tensor must exceed G.
(b) Inference per (config, engine): pred_t, pred_v, nsp, seq_out_t (valid rows) against the float64 oracle, on the default
    schedule and on the padded one that collects probabilities.  fp32x3: |err| <= 1e-3 + 1e-3 |want| (`close` of
    tests/test_gpu_x3_model.py).  bf16: what the full config's own test of these outputs applies
    (test_full_config_b6_matches_reference_golden, tests/test_gpu_model.py; tests/test_gpu_fullsize.py reads only losses and NSP
    logits against the oracle, at 1e-2 + 1e-2 |want|, which is the NSP gate here too): |err| <= 1e-2 max(1, max |want|), and in
    the allclose form 1e-2 + 1e-2 |want| at least 99.5 % of the elements inside with a worst ratio of 2 (pred_t; pred_v by the
    same rule) / 98 % and 4 (seq_out_t).  The attention probabilities of output_all_attention_masks=True: [B, heads, Tq, Tk]
    with this configuration's head counts, rows with a valid key sum to 1 over the valid keys within 1e-3, masked keys exactly 0.
(c) The call forms with a narrower envelope than the config check.  Read from the entry checks of csrc/attention.hip
    (`attn_spliced_fwd_entry`, `attn_spliced_bwd_entry`: D == 64; `fill_fwd`, which unimm_attn_fwd with a shared segment goes
    through: 64 or 128), csrc/x3ops.hip (`fill_attn`: 64 or 128) and csrc/generate.hip (unimm_attn_decode: 64):

      form                                       engine   text head 64 (narrow, odd)   text head 128 (swapped, wide)
      sequence_log_likelihood(shared_context=)   bf16     runs                         runs  (unimm_attn_fwd, shared segment)
      sequence_log_likelihood(shared_context=)   fp32x3   runs                         runs  (unimm_x3_attn_fwd)
      forward_backward(shared_context=)          bf16     runs                         ValueError naming the head size
      forward_backward(shared_context=)          fp32x3   ValueError: the step runs on the bf16 engine only (any head size)
      generate_answers                           bf16     runs                         ValueError naming the head size
      generate_answers                           fp32x3   NotImplementedError: generation runs on the bf16 engine (any head size)

    Every refusal is raised on the host before anything is launched (the test holds the library's call counter still across
    it); nothing raises UnimmHipError.  The image and connection head sizes restrict no form.

Measured (MI355X; the tests print the per-family tables):
  (a) worst relative L2 of a live tensor, and the negative control (worst live tensor against the oracle mutated at the text
      site / at the connection site; G = 0.1323)
        config    bf16       fp32x3     control bf16     control fp32x3
        swapped   1.14e-2    1.34e-5    0.422 / 0.435    0.422 / 0.435
        narrow    1.15e-1    1.42e-5    0.553 / 0.499    0.555 / 0.498
        wide      3.58e-2    5.06e-5    0.529 / 0.581    0.529 / 0.581
        odd       1.17e-2    1.44e-5    0.483 / 0.495    0.484 / 0.495
      narrow / bf16 is at 0.87 G on ONE tensor, bert.v_pooler.dense.bias (64 elements; norm error 0.7 %, worst element 14 % of the
      largest; every other family <= 2.3e-2): a ReLU unit of the image pooler whose pre-activation lies within the bf16 noise of
      zero for one of the 6 sequences gains or loses that sequence's whole contribution -- what tests/test_gpu_fullsize.py
      describes for the poolers at full size; fp32x3 on the same case and masks is at 1.4e-5.  No exception was needed.
  (b) bf16, worst |err| / (1e-2 + 1e-2 |want|) of pred_t / pred_v / seq_out_t / nsp (all elements inside the allclose form but one
      family): swapped 0.47 / 0.36 / 0.28 / 0.005, narrow 0.27 / 0.37 / 0.04 / 0.000, wide 0.90 / 1.09 / 0.55 / 0.073,
      odd 0.45 / 0.82 / 0.40 / 0.008; wide pred_v: max |err| 1.16e-2 on scale 2.61.  fp32x3: at most 0.020 of its gate.
      Probabilities: worst |sum - 1| 2.4e-7, masked keys 0.
  (c) shared scores against the oracle, bf16: at most 7.3e-3 on scale 68 (wide); fp32x3: 2.7e-5.  Against the per-candidate path:
      bf16 5.5e-3 (swapped), bit-equal elsewhere; fp32x3 7.6e-6.  Shared training step (narrow, odd): loss equal to the
      replicated step's to 7 digits, gradient arenas apart by 2.8e-5 / 2.3e-4 of the replicated norm.  generate_answers (narrow,
      odd): worst step log p at 0.018 / 0.035 of 1e-2 + 1e-2 |want|.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import vilbert_ref as R
from tests import envelope_case as EC
from tests import grad_ref as GR
from tests.test_gpu_fullsize import CLASS_TOL
from tests.test_gpu_model import close as close_bf16
from tests.test_gpu_train_grads import EXCEPTIONS, LOSS_TOL, X3_GATE, _close, _report, _train_steps
from tests.test_gpu_x3_model import close

pytestmark = pytest.mark.gpu

ENGINES = ("bf16", "fp32x3")
RUNS = [(c, e) for c in EC.IDS for e in ENGINES]
RUN_IDS = [f"{c}-{e}" for c, e in RUNS]
SCORE_TOL = {"bf16": 1e-2, "fp32x3": 1e-3}          # candidate log-likelihoods: tests/test_gpu_model.py (1e-2 of the largest) / close()
SHARED_LOSS_TOL = 2e-3                              # tests/test_gpu_shared_training.py: shared against replicated loss


@pytest.fixture(scope="module")
def models():
    """One model per (config, engine), built on first use."""
    from unimm_amd import BertForMultiModalPreTraining
    built = {}

    def get(case, compute):
        if (case, compute) not in built:
            c = EC.build(case)
            model = BertForMultiModalPreTraining(c["cfg"], compute_dtype=compute)
            model.load_state_dict(c["sd"], strict=True)
            built[case, compute] = model.cuda().eval()
        return built[case, compute]
    return get


# ---- (a) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,compute", RUNS, ids=RUN_IDS)
def test_training_step_gradients_match_the_mask_replaying_oracle(models, case, compute):
    c = EC.build(case)
    G = GR.gate()
    model = models(case, compute)
    got, plan, pruned = _train_steps(model, c["args"], c["kw"], {}, 1)
    want = c["base"]
    print(f"\n{case} / {compute}: step {EC.STEP}, last text layer {'on the loss rows' if pruned else 'on all rows'}")

    # ---- the plan: the step ran on the valid rows, numbered as the replay numbered them
    assert plan is not None and plan["Mv"] == c["Mv"] == 341 and EC.N_SEQ * EC.T == 480
    assert torch.equal(plan["rows"][:c["Mv"]], c["rows"]) and sum(plan["lens_h"]) == c["Mv"]
    assert pruned == (compute == "bf16")
    assert want["sites"] == GR.site_names(c["ocfg"])

    # ---- losses and scores
    tol = LOSS_TOL[compute]
    for k in ("lm_loss", "img_loss", "nsp_loss"):
        _close(got["losses"][k], want["losses"][k], tol, k)
    _close(got["nsp"], want["nsp"], tol, "nsp scores")

    # ---- gradients
    for n, w in want["grads"].items():
        assert (got["grads"][n] is None) == (w is None), (n, "oracle has no gradient" if w is None else "oracle has a gradient")
    assert set(got["grads"]) - set(want["grads"]) <= {R.TIED[0]}
    cmp = GR.compare(got["grads"], want["grads"])
    _report(cmp, f"{case} / {compute}")
    top = max(v["want_norm"] for v in cmp.values())
    dead = [n for n, v in cmp.items() if v["dead"]]
    for n in dead:
        assert cmp[n]["norm"] <= GR.DEAD_NORM_BOUND * top, (n, cmp[n])
    live = {n: v for n, v in cmp.items() if not v["dead"]}
    assert (len(live), len(dead)) == EC.LIVE_DEAD[case], (len(live), len(dead))
    if compute == "fp32x3":
        bad = {n: v["l2"] for n, v in live.items() if v["l2"] > X3_GATE}
    else:
        assert len(EXCEPTIONS) <= 0.1 * len(live)
        bad = {n: v["l2"] for n, v in live.items() if v["l2"] > (EXCEPTIONS[n][0] if n in EXCEPTIONS else G)}
    assert not bad, (f"gate {X3_GATE if compute == 'fp32x3' else G:.4g}", sorted(bad.items(), key=lambda kv: -kv[1])[:8])

    # ---- negative control: a wrong mask at either of two sites of the oracle must show on some live tensor
    gate = X3_GATE if compute == "fp32x3" else G
    for site in EC.control_sites(c["ocfg"]):
        mut = EC.oracle_run(c, {site: "key"})
        cm = {n: v for n, v in GR.compare(got["grads"], mut["grads"]).items() if not v["dead"]}
        worst = max(cm, key=lambda n: cm[n]["l2"])
        print(f"  control: oracle mutated at {site}: worst live tensor {worst} relative L2 {cm[worst]['l2']:.4f} (G {G:.4f}); "
              f"tensors above their gate: {sum(v['l2'] > gate for v in cm.values())}")
        assert cm[worst]["l2"] > G, (site, worst, cm[worst])


# ---- (b) -----------------------------------------------------------------------------------------------------------------------
_ORACLE_INF = {}


def _oracle_inference(c):
    """The float64 oracle's inference outputs of the case's batch, once per case."""
    if c["id"] not in _ORACLE_INF:
        f64 = lambda v: v.double() if torch.is_tensor(v) and v.is_floating_point() else v
        sd = {k: v.double() for k, v in c["sd"].items()}
        kw = {k: f64(c["kw"][k]) for k in ("token_type_ids", "position_ids", "attention_mask", "image_attention_mask", "co_attention_mask")}
        with torch.no_grad():
            _ORACLE_INF[c["id"]] = R.forward(sd, c["ocfg"], *[f64(a) for a in c["args"]], **kw)
    return _ORACLE_INF[c["id"]]


def _probs_ok(p, heads, Tq, Tk, mask, what):
    """p [B, heads, Tq, Tk]; mask [B, Tq, Tk] or [B, Tk] of 0 / 1: rows with a valid key sum to 1 over the valid keys, masked keys
    are exactly 0 there.  (Rows without one: the reference takes the softmax of the raw scores; not looked at.)"""
    B = mask.shape[0]
    assert tuple(p.shape) == (B, heads, Tq, Tk), (what, tuple(p.shape), (B, heads, Tq, Tk))
    m = mask.to(p.device).bool()
    m = (m[:, None, :] if m.dim() == 2 else m)[:, None].expand(B, heads, Tq, Tk)
    rows = m.any(-1)
    assert bool(rows.any())
    assert torch.isfinite(p).all()
    s = (p * m).sum(-1)[rows]
    worst = float((s - 1).abs().max())
    leaked = float((p * ~m).abs().amax(-1)[rows].max())
    print(f"  {what}: {int(rows.sum())} rows with a valid key, worst |sum - 1| {worst:.2e}, largest masked probability {leaked:.1e}")
    assert worst <= 1e-3 and leaked == 0.0, (what, worst, leaked)


@pytest.mark.parametrize("case,compute", RUNS, ids=RUN_IDS)
def test_inference_matches_the_oracle_and_attention_probabilities_are_distributions(models, case, compute):
    c = EC.build(case)
    cfg = c["cfg"]
    model = models(case, compute)
    model.eval()
    want = _oracle_inference(c)
    kw = {k: c["kw"][k] for k in ("token_type_ids", "position_ids", "attention_mask", "image_attention_mask", "co_attention_mask")}
    with torch.no_grad():
        plain = model(*c["args"], **kw)
        probed = model(*c["args"], **kw, output_all_attention_masks=True)
    torch.cuda.synchronize()
    assert plain[4] == ([], [], [])
    tol = CLASS_TOL[compute]
    rows = c["rows"]
    B, T, Rg = EC.N_SEQ, EC.T, EC.REGIONS
    print()
    for out, tag in ((plain, "default schedule"), (probed, "padded schedule with probabilities")):
        pred_t, pred_v, nsp, seq_t = out[:4]
        assert tuple(pred_t.shape) == (B, T, cfg.vocab_size) and tuple(pred_v.shape) == (B, Rg, cfg.v_target_size)
        assert tuple(seq_t.shape) == (B, T, cfg.hidden_size) and tuple(nsp.shape) == (B, 2)
        flat = lambda x: x.reshape(B * T, -1).cpu()[rows]
        what = lambda name: f"{case} / {compute} {name} ({tag})"
        if compute == "fp32x3":
            close(flat(pred_t), flat(want["pred_t"]), tol, what("pred_t"))
            close(pred_v, want["pred_v"], tol, what("pred_v"))
            close(flat(seq_t), flat(want["seq_out_t"]), tol, what("seq_out_t"))
        else:
            # the full config's rule for these outputs (test_full_config_b6_matches_reference_golden): |err| <= 1e-2 max(1, max |want|),
            # and in the allclose form 1e-2 + 1e-2 |want| a share of the elements inside and a bound on the worst ratio; pred_v, which
            # that test does not read, by the rule of the other head's logits
            f64 = lambda x: x.double().numpy()
            close_bf16(flat(pred_t), f64(flat(want["pred_t"])), tol, what("pred_t"), scale_rel=True, min_share=0.995, max_ratio=2.0)
            close_bf16(pred_v, f64(want["pred_v"]), tol, what("pred_v"), scale_rel=True, min_share=0.995, max_ratio=2.0)
            close_bf16(flat(seq_t), f64(flat(want["seq_out_t"])), tol, what("seq_out_t"), scale_rel=True, min_share=0.98, max_ratio=4.0)
        close(nsp, want["nsp"], tol, what("nsp"))
        assert torch.isfinite(seq_t).all() and torch.isfinite(pred_t).all()
    att_t, att_v, att_c = probed[4]
    assert len(att_t) == cfg.num_hidden_layers and len(att_v) == cfg.v_num_hidden_layers and len(att_c) == len(cfg.v_biattention_id)
    am, im, co = kw["attention_mask"], kw["image_attention_mask"], kw["co_attention_mask"]
    for i, p in enumerate(att_t):
        _probs_ok(p, cfg.num_attention_heads, T, T, am, f"text layer {i}")
    for i, p in enumerate(att_v):
        _probs_ok(p, cfg.v_num_attention_heads, Rg, Rg, im, f"image layer {i}")
    for i, (p1, p2) in enumerate(att_c):
        _probs_ok(p1, cfg.bi_num_attention_heads, T, Rg, im, f"connection {i}: text attends regions")
        _probs_ok(p2, cfg.bi_num_attention_heads, Rg, T, co, f"connection {i}: regions attend text")


# ---- (c) -----------------------------------------------------------------------------------------------------------------------
FORMS = ("score_shared", "train_shared", "generate")


def expected(form, compute, text_head):
    """The docstring's table: "runs", or (exception types, pattern of the message)."""
    if form == "score_shared":
        return "runs"
    if compute != "bf16":
        return ((ValueError,), "bf16 engine only") if form == "train_shared" else ((NotImplementedError,), "bf16 engine")
    if text_head == 64:
        return "runs"
    return (ValueError,), f"text head size {text_head}"


class _Launches:
    """Counts the calls into the library (unimm_amd.lib._call is the one door every launch goes through)."""

    def __enter__(self):
        from unimm_amd import lib as L
        self.L, self.inner, self.n = L, L._call, 0

        def counted(*a, **k):
            self.n += 1
            return self.inner(*a, **k)
        L._call = counted
        return self

    def __exit__(self, *exc):
        self.L._call = self.inner


def _refused(call, types, pattern):
    from unimm_amd.lib import UnimmHipError
    assert not any(issubclass(t, UnimmHipError) or issubclass(UnimmHipError, t) for t in types)
    with _Launches() as seen:
        with pytest.raises(types, match=pattern) as e:
            call()
    assert not isinstance(e.value, UnimmHipError)
    assert seen.n == 0, f"{seen.n} library calls before the refusal"
    print(f"  refused on the host: {type(e.value).__name__}: {e.value}")


def _scoring_batch(model):
    from unimm_amd import synth
    b = synth.make_scoring_batch(rounds=2, options=3, T=EC.T, R=EC.REGIONS, cfg=model.config, seed=7, a_range=(1, 10), c_range=(10, 40),
                                 device="cuda")
    b.pop("mask_spec")
    args = (b["input_ids"], b["image_feat"], b["image_loc"], b["masked_lm_labels"])
    kw = dict(token_type_ids=b["token_type_ids"], position_ids=b["token_position_ids"], attention_mask=b["attention_mask"],
              co_attention_mask=b["co_attention_mask"], image_attention_mask=b["image_attention_mask"])
    return b, args, kw


def _score_shared(model, c, compute):
    from tests.test_gpu_x3_scoring import oracle_scores
    b, args, kw = _scoring_batch(model)
    grp = b["context_group"]
    from unimm_amd import scoring
    plans, inner = [], scoring.forward_shared
    scoring.forward_shared = lambda *a, **k: (plans.append(inner(*a, **k)), plans[-1])[1]
    try:
        got, nsp = model.sequence_log_likelihood(*args, shared_context=grp, **kw)
        assert len(plans) == 1 and plans[0]["plan"].G == 2 and bool(plans[0]["ok"].all())     # the shared pass ran, on two groups
        base, nsp0 = model.sequence_log_likelihood(*args, **kw)
        assert len(plans) == 1                                                                  # ... and the per-candidate path is another
    finally:
        scoring.forward_shared = inner
    torch.cuda.synchronize()
    assert got.shape == (6,) and torch.isfinite(got).all() and (got < 0).all()
    want, want_nsp = oracle_scores(c["ocfg"], c["sd"], b)
    scale = float(want.abs().max())
    d_o, d_b = float((got.cpu() - want).abs().max()), float((got - base).abs().max())
    print(f"  shared scores: vs oracle {d_o:.3e}, vs per-candidate {d_b:.3e} on scale {scale:.3g}; NSP vs oracle "
          f"{float((nsp.cpu() - want_nsp).abs().max()):.3e}, vs per-candidate {float((nsp - nsp0).abs().max()):.3e}")
    if compute == "fp32x3":
        close(got, want, what="shared scores vs oracle")
        close(got, base.cpu(), what="shared vs per-candidate scores")
        close(nsp, want_nsp, what="shared NSP logits vs oracle")
        close(nsp, nsp0.cpu(), what="shared vs per-candidate NSP logits")
    else:
        assert d_o <= SCORE_TOL["bf16"] * scale, (d_o, scale)                  # tests/test_gpu_model.py: 1e-2 of the largest |score|
        assert d_b <= 2e-3 * float(base.abs().max())                           # tests/test_gpu_x3_scoring.py, bf16
        close(nsp, want_nsp, CLASS_TOL["bf16"], what="shared NSP logits vs oracle")
        assert float((nsp - nsp0).abs().max()) <= 2e-2 * (1 + float(nsp0.abs().max()))


def _dialogs(model, G, seed):
    from tests.test_gpu_generate import make_dialogs
    cfg = model.config
    d, ctx, utts = make_dialogs(G, EC.T, cfg.vocab_size, EC.REGIONS, cfg.v_feature_size, seed=seed, cmin=8, cmax=40)
    assert len(set(int(x) for x in ctx)) == G, ctx                               # contexts of different lengths
    return d, ctx, utts


def _train_shared_call(model, shared):
    """-> a call of forward_backward on 3 dialogs x 3 sampled answers of 1 .. 6 tokens, replicated or on the shared schedule"""
    from tests.test_gpu_policy_model import policy_inputs
    from unimm_amd.policy import sampled_training_batch
    G, N = 3, 3
    d, ctx, _ = _dialogs(model, G, seed=21)
    rng = np.random.default_rng(3)
    lengths = rng.integers(1, 7, size=(G, N))
    lengths[0, 0], lengths[-1, -1] = 1, 6
    ans = SimpleNamespace(tokens=torch.from_numpy(rng.integers(110, 1000, size=(G, N, 6))), lengths=torch.from_numpy(lengths))
    sb = sampled_training_batch(d["input_ids"], d["token_type_ids"], d["position_ids"], ctx, ans, EC.T)
    kw = policy_inputs(sb, d, G, model.config.v_target_size)
    if shared:
        kw["shared_context"] = sb.image_index
    return lambda: model.forward_backward(sb.input_ids, d["image_feat"], d["image_loc"], (1.0, 0.0, 0.0), **kw)


DROPOUTS = ("hidden_dropout_prob", "attention_probs_dropout_prob", "v_hidden_dropout_prob", "v_attention_probs_dropout_prob")


def _train_shared(model):
    """The loss of the shared step against the replicated step's, dropout off (tests/test_gpu_shared_training.py (a))."""
    eng = model.engine
    eng.ensure(torch.device("cuda", 0))
    was = {k: getattr(model.config, k) for k in DROPOUTS}
    model.train()
    try:
        for k in DROPOUTS:
            setattr(model.config, k, 0.0)
            setattr(eng.cfg, k, 0.0)
        res = {}
        for shared in (False, True):
            model.set_dropout_seed(9, 0)
            eng.arena.zero_grads()
            out = _train_shared_call(model, shared)()
            torch.cuda.synchronize()
            res[shared] = (float(out[1]), eng.arena.grad_flat.clone())
    finally:
        for k, v in was.items():
            setattr(model.config, k, v)
            setattr(eng.cfg, k, v)
        eng.arena.zero_grads()
        model.zero_grad(set_to_none=True)
        model.eval()
    (lm_r, g_r), (lm_s, g_s) = res[False], res[True]
    d = float((g_s - g_r).norm() / g_r.norm())
    print(f"  shared training step: loss replicated {lm_r:.6f} shared {lm_s:.6f}; |g_shared - g_replicated| / |g_replicated| {d:.3e}")
    assert math.isfinite(lm_s) and abs(lm_s - lm_r) <= SHARED_LOSS_TOL * abs(lm_r), (lm_s, lm_r)
    assert torch.isfinite(g_s).all() and float(g_r.norm()) > 0


def _generate(model, c):
    """beams = 2, four tokens at most, teacher-forced against the oracle (tests/test_gpu_generate.py, tiny config)."""
    from tests.test_gpu_generate import SEP, answers_of, gen_kwargs, oracle_steps
    G, beams = 3, 2
    d, ctx, utts = _dialogs(model, G, seed=2)
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], ctx, beams=beams, max_answer_len=4, **gen_kwargs(d))
    torch.cuda.synchronize()
    idx, answers, rows = [], [], []
    for g in range(G):
        for b in range(beams):
            ans, n = answers_of(res, g, b)
            assert 2 <= n <= 5 and res.tokens[g, b, n - 1] == SEP and not set(ans) & {0, 101, 103, SEP}
            idx.append(g)
            answers.append(ans)
            rows.append((g, b, n))
    steps = oracle_steps(c["ocfg"], c["sd"], d, idx, utts, answers, EC.T)
    worst = 0.0
    for (g, b, n), ans, lp in zip(rows, answers, steps):
        want = torch.stack([lp[k, t] for k, t in enumerate(ans + [SEP])])
        got = res.step_logp[g, b, :n].double().cpu()
        worst = max(worst, float(((got - want).abs() / (1e-2 + 1e-2 * want.abs())).max()))
        assert ((got - want).abs() <= 1e-2 + 1e-2 * want.abs()).all(), (g, b, got, want)
        assert abs(float(res.logp[g, b]) - float(want.sum())) <= 1e-2 * n + 1e-2 * abs(float(want.sum()))
    print(f"  generate_answers: {len(rows)} hypotheses, worst |err| / (1e-2 + 1e-2 |want|) of a step's log p {worst:.3f}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case,compute", RUNS, ids=RUN_IDS)
def test_narrower_call_forms_run_or_refuse_on_the_host(models, case, compute, form):
    c = EC.build(case)
    model = models(case, compute)
    text_head = EC.HEAD_SIZES[case][0]
    what = expected(form, compute, text_head)
    print(f"\n{case} / {compute} / {form}: text head size {text_head} -> {what if what == 'runs' else 'refuses'}")
    model.eval()
    if what == "runs":
        if form == "score_shared":
            _score_shared(model, c, compute)
        elif form == "train_shared":
            _train_shared(model)
        else:
            _generate(model, c)
        return
    types, pattern = what
    if form == "train_shared":
        model.engine.ensure(torch.device("cuda", 0))
        model.train()
        try:
            _refused(_train_shared_call(model, True), types, pattern)
        finally:
            model.eval()
    else:
        assert form == "generate"
        from tests.test_gpu_generate import gen_kwargs
        d, ctx, _ = _dialogs(model, 3, seed=2)
        _refused(lambda: model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], ctx, beams=2, max_answer_len=4,
                                                **gen_kwargs(d)), types, pattern)

