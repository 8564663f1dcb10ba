"""The CIDEr-D reward through its Python surface on the small configuration of tests/test_gpu_policy_model.py: `CiderD.score` on
what `generate_answers` returns, `trainer.self_critical_step` with a `CiderD` against the same step driven by a host callable that
wraps tests/reward_ref.py, the step with a plain callable (launch for launch what it is without the feature, the extension library
never touched), and `metrics.cider_d` on a beam result.  Rewards are compared within one fp32 ulp of float32(reference), the bound
of tests/test_gpu_reward_edges.py."""
import numpy as np
import pytest
import torch

from tests import reward_ref as RR
from tests.test_gpu_generate import gen_kwargs, tiny  # noqa: F401
from tests.test_gpu_policy_model import MAXLEN, _encoder, tiny_dialogs

pytestmark = pytest.mark.gpu


def generate(model, d, c, **kw):
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, **gen_kwargs(d), max_answer_len=MAXLEN, **kw)
    torch.cuda.synchronize()
    return res


def references_from(results, weights_seed):
    """[G, M, W] references out of generated answers: every answer of every result, the second one cut by a token, one absent
    row at the end; weights with a zero among them"""
    toks = torch.cat([r.tokens for r in results], dim=1).cpu().clone()
    lens = torch.cat([r.lengths for r in results], dim=1).cpu().clone()
    G, M, W = toks.shape
    for g in range(G):
        n = int(lens[g, 1])
        if n > 2:                                                           # drop the last token: [.., t, SEP] -> [.., SEP, 0]
            toks[g, 1, n - 2], toks[g, 1, n - 1], lens[g, 1] = toks[g, 1, n - 1], 0, n - 1
    toks = torch.cat([toks, torch.full((G, 1, W), 7, dtype=toks.dtype)], dim=1)
    lens = torch.cat([lens, torch.zeros((G, 1), dtype=lens.dtype)], dim=1)
    w = torch.rand((G, M + 1), generator=torch.Generator().manual_seed(weights_seed)) + 0.25
    w[:, 2] = 0.0
    return toks, lens, w


def host_idf(table):
    return RR.table_idf(table.keys.cpu().numpy(), table.idf.cpu().numpy(), table.default_idf)


def ulps(got, want64):
    want32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    got = np.asarray(got, dtype=np.float32)
    return np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


def test_score_on_a_rollout_equals_the_reference(tiny):
    from unimm_amd import reward
    model, _, _ = tiny
    d, c, _ = tiny_dialogs(G=4, seed=8)
    res = generate(model, d, c, samples=4, greedy=True, seed=3)
    rt, rl, rw = references_from([generate(model, d, c, samples=3, seed=9), res.greedy], 1)
    table = reward.NgramTable.from_corpus(rt.reshape(-1, rt.shape[-1]), rl.reshape(-1))
    assert table.device.type == "cuda"
    for tab, idf in ((table, host_idf(table)), (None, RR.unit_idf)):
        scorer = reward.CiderD(tab)
        got = scorer.score(res.tokens, res.lengths, rt, rl, rw)            # device answers, host references
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(res.lengths.shape)
        want = RR.score(res.tokens.tolist(), res.lengths.tolist(), rt.tolist(), rl.tolist(), rw.double().tolist(), idf)
        u = ulps(got.cpu().numpy(), want)
        print(f"\nsamples: reward {want.min():.4f} .. {want.max():.4f}, off by at most {u.max():.2f} fp32 ulp (table: {tab is not None})")
        assert (u <= 1.0).all() and (want > 0).any()
        greedy = scorer.score(res.greedy.tokens.int().cpu(), res.greedy.lengths.int(), rt.cuda(), rl.cuda(), rw.cuda())
        want = RR.score(res.greedy.tokens.tolist(), res.greedy.lengths.tolist(), rt.tolist(), rl.tolist(), rw.double().tolist(), idf)
        assert (ulps(greedy.cpu().numpy(), want) <= 1.0).all() and (want > 0).all()       # the greedy answer is a reference
        flat, orders = scorer.score_rows(res.tokens.reshape(-1, res.tokens.shape[-1]), res.lengths.reshape(-1),
                                         torch.arange(4).repeat_interleave(4), rt, rl, rw, per_order=True)
        assert torch.equal(flat.view(4, 4), got) and tuple(orders.shape) == (16, 4) and orders.dtype == torch.float64
    moved = reward.NgramTable.from_corpus(rt.reshape(-1, rt.shape[-1]), rl.reshape(-1), device="cpu")
    moved.load_state_dict(table.state_dict())
    assert torch.equal(reward.CiderD(moved.to("cuda")).score(res.tokens, res.lengths, rt, rl, rw),
                       reward.CiderD(table).score(res.tokens, res.lengths, rt, rl, rw))


def recorded_step(monkeypatch, reward_fn, batch, forbid_extension, **kw):
    """(the step's result, the launch profiler's GEMM counts, the C entry points in call order, the generate_answers results)"""
    from unimm_amd import lib as L
    from unimm_amd import mix as MX
    from unimm_amd import reward_abi as RA
    from unimm_amd import trainer
    enc, opt, sch = _encoder()
    eng = enc.bert_pretrained.engine
    eng.ensure(torch.device("cuda", 0))
    p0 = eng.arena.flat.clone()
    answers, real = [], enc.generate_answers
    enc.generate_answers = lambda *a, **k: (answers.append(real(*a, **k)), answers[-1])[1]
    with monkeypatch.context() as mp:
        calls = []
        for mod in (L, MX, RA):
            mp.setattr(mod, "_call", lambda name, *a, real=mod._call: (calls.append(name), real(name, *a))[1])
        if forbid_extension:
            mp.setattr(RA, "lib", lambda: pytest.fail("a step with a host reward touched the extension library"))
        L.prof_enable(True)
        try:
            out = trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), 1, reward_fn, samples=3,
                                             baseline="greedy", max_answer_len=MAXLEN, seed=4, **kw)
            torch.cuda.synchronize()
            prof = {k: v[2] for k, v in L.prof_collect().items()}
        finally:
            L.prof_enable(False)
    assert not torch.equal(p0, eng.arena.flat) and torch.isfinite(eng.arena.flat).all()
    return out, prof, [n for n in calls if not n.startswith("unimm_prof")], answers


@pytest.fixture(scope="module")
def step_world():
    """the dialogs of the step tests and references made of the encoder's own answers (its samples at the step's seed and its
    greedy answer), so that the rewards and the baseline are far from zero"""
    from unimm_amd import reward
    d, c, _ = tiny_dialogs(G=4, seed=8)
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"])
    enc, _, _ = _encoder()
    enc.eval()
    rt, rl, rw = references_from([generate(enc, d, c, samples=3, seed=4), generate(enc, d, c, beams=1)], 2)
    table = reward.NgramTable.from_corpus(rt.reshape(-1, rt.shape[-1]), rl.reshape(-1))
    return dict(batch, reference_tokens=rt, reference_lengths=rl, reference_weights=rw), table


@pytest.mark.parametrize("rollout, shared_context", [("separate", False), ("fused", False), ("separate", True), ("fused", True)])
def test_self_critical_step_with_cider_d_is_the_step_with_the_host_reference(step_world, monkeypatch, rollout, shared_context):
    from unimm_amd import reward
    batch, table = step_world
    idf = host_idf(table)
    rt, rl, rw = batch["reference_tokens"], batch["reference_lengths"], batch["reference_weights"]
    seen = {"host": [], "device": []}

    def host_reward(tokens, lengths):
        assert not tokens.is_cuda and not lengths.is_cuda
        r = RR.score(tokens.tolist(), lengths.tolist(), rt.tolist(), rl.tolist(), rw.double().tolist(), idf)
        seen["host"].append(r)
        return torch.from_numpy(r.astype(np.float32))

    class Spy(reward.CiderD):
        def score(self, tokens, lengths, *refs):
            assert tokens.is_cuda and lengths.is_cuda and refs[0] is rt and refs[1] is rl and refs[2] is rw
            out = super().score(tokens, lengths, *refs)
            assert out.is_cuda
            seen["device"].append(out.cpu().numpy())
            return out

    plain = {k: v for k, v in batch.items() if not k.startswith("reference_")}     # a host reward needs no reference keys
    kw = dict(rollout=rollout, shared_context=shared_context)
    a = recorded_step(monkeypatch, host_reward, plain, True, **kw)
    b = recorded_step(monkeypatch, Spy(table), batch, False, **kw)
    # the rollouts are the same draws, and the device reward saw them where they are
    assert len(a[3]) == len(b[3]) == (1 if rollout == "fused" else 2)
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x.tokens, y.tokens) and torch.equal(x.lengths, y.lengths)
    assert len(seen["host"]) == len(seen["device"]) == 2                    # the samples, then the greedy baseline
    worst, same_bits, top = 0.0, True, 0.0
    for h, dv in zip(seen["host"], seen["device"]):
        assert h.shape == dv.shape
        worst = max(worst, float(ulps(dv, h).max()))
        same_bits = same_bits and h.astype(np.float32).tobytes() == dv.tobytes()
        top = max(top, float(np.abs(h).max()))
    (loss_a, reward_a, base_a, ent_a), (loss_b, reward_b, base_b, ent_b) = a[0], b[0]
    print(f"\n{rollout}, shared_context={shared_context}: loss {loss_a:.6f} / {loss_b:.6f}, reward {reward_a:.4f} / {reward_b:.4f}, "
          f"baseline {base_a:.4f} / {base_b:.4f}; rewards off by at most {worst:.2f} fp32 ulp, equal bits: {same_bits}")
    assert worst <= 1.0
    assert reward_a > 0 and base_a > 0, "the references were chosen to overlap"
    one_ulp = float(np.spacing(np.float32(top)))
    assert abs(reward_a - reward_b) <= one_ulp and abs(base_a - base_b) <= 2 * one_ulp      # the baseline: a difference of two
    if same_bits:                                                           # equal inputs: equal bits, as test_gpu_policy_model.py asks
        assert (loss_a, reward_a, base_a, ent_a) == (loss_b, reward_b, base_b, ent_b)
    else:                                                                   # the loss is linear in the advantages, normalised by a count
        mass = float(a[3][0].step_logp.abs().sum())
        assert abs(loss_a - loss_b) <= 2 * one_ulp * mass
    # launch for launch: what the host-reward step called, plus the two reward launches
    assert a[1] == b[1] and sum(a[1].values()) > 0
    assert "unimm_ngram_reward" not in a[2] and b[2].count("unimm_ngram_reward") == 2
    assert a[2] == [n for n in b[2] if n != "unimm_ngram_reward"]


def test_a_missing_reference_key_raises_before_the_rollout(step_world):
    from unimm_amd import reward, trainer
    batch, table = step_world
    enc, opt, sch = _encoder()
    enc.generate_answers = lambda *a, **k: pytest.fail("the rollout ran")
    short = {k: v for k, v in batch.items() if k != "reference_lengths"}
    with pytest.raises(ValueError, match="reference_lengths"):
        trainer.self_critical_step(enc, opt, sch, short, dict(batch_multiply=1), 1, reward.CiderD(table), samples=3,
                                   max_answer_len=MAXLEN, seed=4)


def test_cider_d_metric_on_a_beam_result(tiny):
    from unimm_amd import metrics, reward
    model, _, _ = tiny
    d, c, _ = tiny_dialogs(G=4, seed=8)
    res = generate(model, d, c, beams=3)
    rt, rl, rw = references_from([generate(model, d, c, samples=3, seed=9), generate(model, d, c, beams=1)], 3)
    table = reward.NgramTable.from_corpus(rt.reshape(-1, rt.shape[-1]), rl.reshape(-1))
    mean, values = metrics.cider_d(res, None, rt, rl, rw, table=table)
    want = RR.score(res.tokens.tolist(), res.lengths.tolist(), rt.tolist(), rl.tolist(), rw.double().tolist(), host_idf(table))
    assert tuple(values.shape) == tuple(res.lengths.shape) == (4, 3) and (ulps(values.cpu().numpy(), want) <= 1.0).all()
    present = (res.lengths > 0).cpu().numpy()
    assert present.all() and abs(mean - float(values.double().mean())) <= 1e-12 and (want[:, 0] > 0).all()
    print(f"\nbeams = 3: CIDEr-D mean {mean:.4f}, best beam {float(values[:, 0].mean()):.4f}")
    # the tokens / lengths form, one hypothesis per dialog, uniform weights, no table
    mean1, values1 = metrics.cider_d(res.tokens[:, 0], res.lengths[:, 0], rt, rl)
    want1 = RR.score(res.tokens[:, :1].tolist(), res.lengths[:, :1].tolist(), rt.tolist(), rl.tolist())
    assert tuple(values1.shape) == (4,) and (ulps(values1.cpu().numpy(), want1[:, 0]) <= 1.0).all()
    assert abs(mean1 - float(values1.double().mean())) <= 1e-12
