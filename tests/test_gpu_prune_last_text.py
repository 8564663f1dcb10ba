"""The last text layer on the rows the training losses read (Engine.prune_last_text): one training step of the small
config, B = 4, with the switch on and with it off, same weights, same dropout seed.

Only the order of some fp32 sums may differ between the two: every row the losses read goes through the same row-wise
kernels with the same dropout masks, so the forward is expected to be bit-equal, and the parameter gradients are bounded by
what a change of the weight-gradient reduction schedule alone does to the switch-off step (measured in the test, 4x margin)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, R = 4, 64, 37


def _build(golden_dir, compute="bf16"):
    from oracle import vilbert_ref as R_
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    cfgd = json.load(open(os.path.join(golden_dir, "small_config.json")))
    model = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd), compute_dtype=compute)
    model.load_state_dict(R_.init_state_dict(R_.make_config(cfgd), seed=11), strict=True)
    model = model.cuda()
    model.engine.ensure(torch.device("cuda", 0))
    return model


def _batch(cfg, seed=7):
    """B = 4 sequences, lengths not all divisible by 32, sequence 1 with a label (and a likelihood weight) on its first token."""
    from unimm_amd import synth
    b = synth.make_batch(n_seq=B, T=T, R=R, cfg=cfg, seed=seed, device="cuda")
    b["masked_lm_labels"][1, 0] = 123
    b["lm_weight"][1, 0] = 1
    return b


def _kw(b):
    return dict(token_type_ids=b["token_type_ids"], position_ids=b["token_position_ids"], attention_mask=b["attention_mask"],
                image_attention_mask=b["image_attention_mask"], co_attention_mask=b["co_attention_mask"],
                masked_lm_labels=b["masked_lm_labels"], image_label=b["image_label"], image_target=b["image_target"],
                next_sentence_label=b["next_sentence_label"], nsp_weight=b["nsp_weight"], lm_weight=b["lm_weight"])


def _step(model, b, want_scores=False):
    """One training step -> (losses [3], NSP logits, {parameter name: gradient or None})."""
    model.train(True)
    model.engine.arena.zero_grads()
    lm, img, nsp_l, _, _, nsp = model(b["input_ids"], b["image_feat"], b["image_loc"], _want_lm_scores=want_scores, **_kw(b))
    (lm + 0.5 * img + 2.0 * nsp_l).sum().backward()
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    return torch.stack([lm, img, nsp_l]).flatten().detach().clone(), nsp.detach().clone(), grads


def _run(golden_dir, b, seed=321, **attrs):
    m = _build(golden_dir)
    m.set_dropout_seed(seed)
    for k, v in attrs.items():
        assert hasattr(m.engine, k), k
        setattr(m.engine, k, v)
    return _step(m, b), m


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-300))


@pytest.fixture(scope="module")
def runs(golden_dir):
    """The steps every test below compares, computed once: switch off / on with split-K off and with default settings, and the
    switch-off step under other weight-gradient reduction schedules."""
    from unimm_amd import BertConfig
    cfg = BertConfig.from_dict(json.load(open(os.path.join(golden_dir, "small_config.json"))))
    b = _batch(cfg)
    out = dict(batch=b)
    (out["off_nosplit"], m) = _run(golden_dir, b, prune_last_text=False, splitk=False)
    plan = m.engine.last_plan
    lens = plan["lens_h"] if plan is not None else [T] * B
    assert any(l % 32 for l in lens), lens                                  # lengths that are no multiple of the attention tile
    (out["on_nosplit"], _) = _run(golden_dir, b, prune_last_text=True, splitk=False)
    (out["off"], _) = _run(golden_dir, b, prune_last_text=False)
    (out["on"], m_on) = _run(golden_dir, b, prune_last_text=True)
    assert m_on.engine.prune_last_text
    (out["off_atomic"], _) = _run(golden_dir, b, prune_last_text=False, wgrad_overwrite=False)
    (out["off_rounds1"], _) = _run(golden_dir, b, prune_last_text=False, wgrad_group_rounds=1)
    return out


def test_forward_is_bit_equal_without_split_k(runs):
    """A row's K reduction does not depend on the tile, the rows keep their dropout masks and the loss sums run over the same
    rows in the same order: the three losses and the NSP logits are the same bits."""
    (l0, n0, _), (l1, n1, _) = runs["off_nosplit"], runs["on_nosplit"]
    print(f"losses off {l0.tolist()} on {l1.tolist()}")
    assert torch.isfinite(l1).all()
    assert torch.equal(l0, l1) and torch.equal(n0, n1)


def test_forward_default_settings(runs):
    """Default settings (split-K allowed): the losses agree within 4x what split-K on / off does to the switch-off step.
    Measured: 0.0 on all three losses -- the small config has no reduction long enough for a split (K <= 256), so this asks
    for bit-equal losses as well."""
    (l_ns, _, _), (l_off, _, _), (l_on, _, _) = runs["off_nosplit"], runs["off"], runs["on"]
    bound = 4.0 * (l_off - l_ns).abs()
    diff = (l_on - l_off).abs()
    print(f"split-K on/off (switch off): {(l_off - l_ns).abs().tolist()}  switch on/off: {diff.tolist()}")
    assert (diff <= bound).all(), (diff.tolist(), bound.tolist())


def test_every_parameter_gradient(runs):
    """Per tensor: None in one path = None in the other, and the relative L2 difference is at most 4x the largest difference
    that another weight-gradient reduction schedule (atomic adds instead of stores into the zeroed arena; one round per grouped
    launch instead of four) makes on any tensor of the switch-off step.
    Measured on MI355X: schedule to schedule 8.6e-8 and 1.19e-7 in two runs (fp32 atomics: it moves), so the bound is 3.4e-7 to
    4.8e-7; switch on against off 1.42e-7 on `bert.encoder.layer.3.output.dense.bias` (a LayerNorm-backward column sum over 57
    loss rows instead of all valid rows) and 0.0 on every other tensor.  A lost contribution -- a first-token gradient, a labelled
    row -- is of order 1e-2 to 1."""
    g_off, g_on = runs["off"][2], runs["on"][2]
    assert set(g_off) == set(g_on)
    base = 0.0
    for other in ("off_atomic", "off_rounds1"):
        g2 = runs[other][2]
        for n, g in g_off.items():
            assert (g is None) == (g2[n] is None), n
            if g is not None and float(g.norm()) > 0:
                base = max(base, _rel_l2(g2[n], g))
    worst = ("", 0.0)
    figures = []
    for n, g in g_off.items():
        assert (g is None) == (g_on[n] is None), n
        if g is None:
            continue
        assert torch.isfinite(g_on[n]).all(), n
        if float(g.norm()) == 0.0:
            assert float(g_on[n].norm()) == 0.0, n
            continue
        d = _rel_l2(g_on[n], g)
        if d > 0.0:
            figures.append((d, n))
        if d > worst[1]:
            worst = (n, d)
    for d, n in sorted(figures, reverse=True):
        print(f"  {d:.3e}  {n}")
    print(f"schedule-to-schedule (switch off): {base:.3e}; switch on/off, worst tensor: {worst[1]:.3e} ({worst[0]})")
    assert worst[1] <= 4.0 * base, (worst, base)


def _launches(fn):
    from unimm_amd import lib as L
    L.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        got = L.prof_collect()
    finally:
        L.prof_enable(False)
    return {k: (round(v[1]), v[2]) for k, v in got.items()}          # variant -> (FLOPs, launches)


def test_inactive_paths_launch_what_they_always_did(golden_dir, runs, monkeypatch):
    """Eval, a step whose caller reads the sequence output / all rows' scores, UNIMM_PRUNE_LAST_TEXT=0 and the fp32x3 engine
    run the launches of the switch-off engine; the training step without sequence output does not (fewer GEMM FLOPs)."""
    b = runs["batch"]
    on, off = _build(golden_dir), _build(golden_dir)
    on.engine.prune_last_text, off.engine.prune_last_text = True, False
    for m in (on, off):
        m.set_dropout_seed(5)
    # the active case, for contrast
    a_on, a_off = _launches(lambda: _step(on, b)), _launches(lambda: _step(off, b))
    assert sum(f for f, _ in a_on.values()) < sum(f for f, _ in a_off.values())
    # a training step that returns the sequence output and every row's scores
    assert _launches(lambda: _step(on, b, want_scores=True)) == _launches(lambda: _step(off, b, want_scores=True))

    def evaluate(m, scores):
        m.train(False)
        with torch.no_grad():
            m(b["input_ids"], b["image_feat"], b["image_loc"], _want_lm_scores=scores, **_kw(b))

    def all_rows(m):                      # lm_rows = "all": no labels -> the inference branch decodes every row
        m.train(False)
        kw = _kw(b)
        kw.update(masked_lm_labels=None, next_sentence_label=None, image_target=None, image_label=None, lm_weight=None)
        with torch.no_grad():
            m(b["input_ids"], b["image_feat"], b["image_loc"], **kw)
    for scores in (False, True):
        assert _launches(lambda: evaluate(on, scores)) == _launches(lambda: evaluate(off, scores))
    assert _launches(lambda: all_rows(on)) == _launches(lambda: all_rows(off))
    # the environment switch, read when the engine is built
    monkeypatch.setenv("UNIMM_PRUNE_LAST_TEXT", "0")
    env = _build(golden_dir)
    monkeypatch.delenv("UNIMM_PRUNE_LAST_TEXT")
    assert env.engine.prune_last_text is False and _build(golden_dir).engine.prune_last_text is True
    env.set_dropout_seed(5)
    assert _launches(lambda: _step(env, b)) == a_off
    # the fp32x3 engine
    x_on, x_off = _build(golden_dir, "fp32x3"), _build(golden_dir, "fp32x3")
    x_on.engine.prune_last_text, x_off.engine.prune_last_text = True, False
    for m in (x_on, x_off):
        m.set_dropout_seed(5)
    r_on, r_off = [None], [None]
    l_on = _launches(lambda: r_on.__setitem__(0, _step(x_on, b)))
    l_off = _launches(lambda: r_off.__setitem__(0, _step(x_off, b)))
    assert l_on == l_off
    assert torch.equal(r_on[0][0], r_off[0][0])


def test_graph_replay_inside_one_capacity_bucket(golden_dir):
    """Two batches with different labelled-row counts that share one capacity bucket replay ONE captured step; the compact
    buffers are sized from the bucket and the real count is read from the device.  Losses as the eager steps give them (fp32
    sums of <= 64 row losses: 2e-6 relative, the bound tests/test_gpu_graphs.py holds the executor to)."""
    from unimm_amd import BertConfig
    cfg = BertConfig.from_dict(json.load(open(os.path.join(golden_dir, "small_config.json"))))
    b1, b2 = _batch(cfg, 7), _batch(cfg, 8)
    ref, gm = _build(golden_dir), _build(golden_dir)
    for m in (ref, gm):
        m.set_dropout_seed(99)
        assert m.engine.prune_last_text
    n1, n2 = (sum(ref.engine.count_rows(b)[B:2 * B]) for b in (b1, b2))          # the plan header: decoded rows per sequence
    assert n1 != n2 and 0 < n1 <= 64 and 0 < n2 <= 64, (n1, n2)
    order = [b1, b2, b1]
    want = [_step(ref, b) for b in order]
    graphs = gm.engine.enable_graphs(row_bucket=B * T, lm_bucket=64, capture_after=0, max_entries=4)
    got = [_step(gm, b) for b in order]
    print(f"labelled rows {n1}, {n2}; executor {graphs.stats}")
    assert len(graphs.entries) == 1 and graphs.stats["replays"] == 3 and graphs.stats["eager"] == 0, graphs.stats
    for i, (w, h) in enumerate(zip(want, got)):
        assert torch.isfinite(h[0]).all(), i
        assert (w[0] - h[0]).abs().max() <= 2e-6 * max(1.0, float(w[0].abs().max())), (i, w[0], h[0])
        assert (w[1] - h[1]).abs().max() <= 2e-6, i
