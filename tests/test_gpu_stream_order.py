"""Cross-stream ordering of every engine schedule, checked on the launch trace of real steps (tests/stream_trace.py records what
is enqueued on which stream with which bytes and which event edges exist; tests/stream_order.py proves every conflicting pair
ordered and every cross-stream use of an allocator block covered).  The streams are real, the verdict does not depend on timing.

A traced case is: arena.zero_grads(), a step, FusedAdamW.step() on the caller's stream, a second step on another batch (host
input cases: four steps, so that a slot of the three-slot staging ring is reused), with no synchronize in between.  The
optimizer runs with lr = 0: its launch, with all its reads and writes, is in the trace, and the parameters keep their bits, so
that the second step's losses can be held to the bit against the default schedule as the first step's are (a non-zero update
would carry the order of the first step's gradient atomics into the second step's parameters).

Every option case is also compared with the default schedule of the same engine under the gate of
test_image_side_stream_schedule_equals_single_stream: losses equal bit for bit, gradients within 1e-5 of the largest gradient.

Negative controls edit the recorded trace, never the run: all waits (or all record_stream calls) issued from one function are
left out, and the checker must then report."""
import os

import pytest
import torch

from tests import stream_order as SO
from tests.stream_trace import Tracer

pytestmark = pytest.mark.gpu
GRAD_TOL = 1e-5
DP_PORT = "29583"

NSP_WEIGHT = torch.tensor([[5.0, 1.0]])          # synth.make_batch's value: a host tensor on every path (the prefetcher gets none)

_CACHE = {}


# ---------------------------------------------------------------------------------------------
# models, batches, steps
# ---------------------------------------------------------------------------------------------
def _model(golden_dir, compute):
    if compute == "fp32x3":
        from tests.test_gpu_x3_model import build_small
    else:
        from tests.test_gpu_model import build_small
    model = build_small(golden_dir)[0]
    model.train()
    model.engine.ensure(torch.device("cuda", 0))
    return model


def _optimizer(model):
    from unimm_amd.optim import FusedAdamW
    return FusedAdamW([dict(params=list(model.parameters()), lr=0.0, weight_decay=0.01)], model.engine, lr=0.0)


def _batches(model, n, device):
    from unimm_amd import synth
    return [synth.make_batch(n_seq=12, T=64, R=37, cfg=model.config, seed=33 + i, sequences_per_image=6, device=device) for i in range(n)]


def _kw(b):
    return dict(token_type_ids=b["token_type_ids"], position_ids=b["token_position_ids"], attention_mask=b["attention_mask"],
                co_attention_mask=b["co_attention_mask"], image_attention_mask=b["image_attention_mask"],
                masked_lm_labels=b["masked_lm_labels"], image_label=b["image_label"], image_target=b["image_target"],
                next_sentence_label=b["next_sentence_label"], nsp_weight=b.get("nsp_weight", NSP_WEIGHT), lm_weight=b["lm_weight"])


def _fb(model, b):
    r = model.forward_backward(b["input_ids"], b["image_feat"], b["image_loc"], (1.0, 1.0, 1.0), **_kw(b))
    return r[1], r[2], r[3]


def _autograd(model, b):
    r = model(b["input_ids"], b["image_feat"], b["image_loc"], **_kw(b), _want_lm_scores=False)
    (r[0] + r[1] + r[2]).sum().backward()
    return r[0].detach(), r[1].detach(), r[2].detach()


def _sequence(model, opt, batches, step=_fb):
    """zero_grads, step, optimizer, the further steps -- nothing in between -> the steps' loss tensors"""
    model.engine.arena.zero_grads()
    out = []
    for i, b in enumerate(batches):
        out.append(step(model, b))
        if i == 0:
            opt.step()
    return out


def _floats(losses):
    return [[float(x.reshape(-1)[0]) for x in step] for step in losses]


def _reference(golden_dir, compute, n):
    """The default schedule of an engine on the first n device-resident batches, untraced -> (losses, gradient arena)"""
    key = ("reference", compute, n)
    if key not in _CACHE:
        model = _model(golden_dir, compute)
        model.set_dropout_seed(5, step=0)
        losses = _sequence(model, _optimizer(model), _batches(model, n, "cuda"))
        torch.cuda.synchronize()
        _CACHE[key] = (_floats(losses), model.engine.arena.grad_flat.clone())
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def _ws_bytes():
    from tests import regime_case as RC
    return RC.ws_bytes_for(RC.build(), {})


CASES = {
    # name: (compute, engine options, entry, parity against the default schedule)
    "bf16": ("bf16", {}, "fb", False),
    "bf16_single_stream": ("bf16", dict(dual_stream=False), "fb", True),
    "bf16_wgrad_stream": ("bf16", dict(wgrad_stream=True), "fb", True),
    "bf16_text_priority": ("bf16", dict(text_priority=True), "fb", True),
    "bf16_image_head_main": ("bf16", dict(image_head_side=False), "fb", True),
    "bf16_wgrad_stream_text_priority": ("bf16", dict(wgrad_stream=True, text_priority=True), "fb", True),
    "bf16_wgrad_ws": ("bf16", dict(wgrad_ws_bytes=_ws_bytes), "fb", True),
    "bf16_autograd": ("bf16", {}, "autograd", False),
    "x3": ("fp32x3", {}, "fb", False),
    "x3_single_stream": ("fp32x3", dict(dual_stream=False), "fb", True),
    "host_stager": ("bf16", dict(host_staging=True), "stager", True),
    "host_prefetcher": ("bf16", {}, "prefetcher", True),
    "shared_context": ("bf16", {}, "shared", False),
    "dp": ("bf16", {}, "dp", True),
    "dp_wgrad_stream": ("bf16", dict(wgrad_stream=True), "dp", True),
}


def _shared_case(tr_factory):
    """forward_backward(shared_context=SharedContext(ids, 64), loss_weights=(1, 0, 0)) on sampled-answer batches"""
    from tests.test_gpu_policy_model import fresh, policy_inputs
    from tests.test_gpu_shared_training import sampled
    from tests.test_gpu_shared_wide_model import ctx64, wide_sampled
    model = fresh()
    model.train()
    model.engine.ensure(torch.device("cuda", 0))
    model.set_dropout_seed(5, step=0)
    opt = _optimizer(model)
    pairs = [wide_sampled(), sampled(4, seed=4)]

    def step(model, pair):
        d, sb = pair
        kw = policy_inputs(sb, d, d["image_feat"].shape[0], model.config.v_target_size)
        r = model.forward_backward(sb.input_ids, d["image_feat"], d["image_loc"], (1.0, 0.0, 0.0), shared_context=ctx64(sb), **kw)
        return r[1], r[2], r[3]
    with tr_factory() as tr:
        losses = _sequence(model, opt, pairs, step)
    torch.cuda.synchronize()
    return tr, model, _floats(losses)


def _traced(name, monkeypatch, golden_dir):
    """Run and trace one case once per process -> dict(tr, an, violations, losses, grads, n)"""
    if name in _CACHE:
        return _CACHE[name]
    compute, opts, entry, _ = CASES[name]
    factory = lambda: Tracer(monkeypatch)
    if entry == "shared":
        tr, model, losses = _shared_case(factory)
        n = 2
    else:
        model = _model(golden_dir, compute)
        eng = model.engine
        for k, v in opts.items():
            assert hasattr(eng, k), k
            setattr(eng, k, v() if callable(v) else v)
        model.set_dropout_seed(5, step=0)
        opt = _optimizer(model)
        n = 4 if entry in ("stager", "prefetcher") else 2
        if entry == "dp":
            import torch.distributed as dist
            from unimm_amd.parallel import DataParallelRCCL
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ["MASTER_PORT"] = DP_PORT
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
            try:
                dp = DataParallelRCCL(model, reduce_when_single=True)
                batches = _batches(model, n, "cuda")
                with factory() as tr:
                    losses = _sequence(model, opt, batches, lambda m, b: _fb(dp, b))
                torch.cuda.synchronize()
                assert dp.comm_stats()["buckets"] == 2 * len(eng.arena.buckets)
            finally:
                eng.grad_bucket_hook = None
                dist.destroy_process_group()
        elif entry == "prefetcher":
            from unimm_amd.inputs import DevicePrefetcher
            host = _batches(model, n, "cpu")
            for b in host:
                assert torch.equal(b.pop("nsp_weight"), NSP_WEIGHT)
            with factory() as tr:
                losses = _sequence(model, opt, DevicePrefetcher(host, torch.device("cuda", 0)))
            torch.cuda.synchronize()
        else:
            batches = _batches(model, n, "cpu" if entry == "stager" else "cuda")
            with factory() as tr:
                losses = _sequence(model, opt, batches, _autograd if entry == "autograd" else _fb)
            torch.cuda.synchronize()
        losses = _floats(losses)
    an = SO.analyse(tr.trace)
    violations = an.check()
    launches, timelines, edges = SO.summary(an)
    print(f"\n{name}: {launches} launches on {timelines} timelines, {edges} cross-stream edges, "
          f"{SO.removable_edges(an) if not violations else '?'} single edges deletable without a report; "
          f"{len(violations)} violations, {len(tr.abi_errors)} ABI errors, {len(tr.thread_errors)} thread errors, "
          f"{len(tr.threads)} launching threads")
    for v in violations[:12]:
        print("   ", an.describe(v))
    for e in (tr.abi_errors + tr.thread_errors)[:12]:
        print("   ", e)
    _CACHE[name] = dict(tr=tr, an=an, violations=violations, losses=losses, grads=model.engine.arena.grad_flat.clone(), n=n,
                        model=model)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_schedule_orders_every_conflicting_pair(name, monkeypatch, golden_dir):
    c = _traced(name, monkeypatch, golden_dir)
    tr, an = c["tr"], c["an"]
    assert not c["violations"], "\n".join(an.describe(v) for v in c["violations"][:20])
    assert not tr.abi_errors, "\n".join(tr.abi_errors[:20])
    # every lib launch arrived on a thread where torch's ops were recorded too (the autograd entry runs the engine's backward
    # on autograd's thread: the engine entry pushes the dispatch mode there, and this check states that it held)
    assert not tr.thread_errors, "\n".join(tr.thread_errors[:20])
    compute, opts, entry, parity = CASES[name]
    device = {t for t in tr.timelines() if t != SO.HOST}
    if opts.get("dual_stream") is False:
        assert len(device) == 1, device                     # exactly one device timeline
    elif entry != "shared":
        assert len(device) >= 2, device                     # the side stream was really used
    if entry == "autograd":
        assert len(tr.threads) >= 1
    if entry == "dp":
        coll = [r for r in tr.trace if r.op == "launch" and r.b.startswith("c10d::")]
        assert coll and all(r.c for r in coll), "no collective in the trace"
        opt_i = next(i for i, r in enumerate(tr.trace) if r.op == "launch" and r.b == "adamw_step")
        assert all(r.a != tr.trace[opt_i].a for r in coll)   # the exchange ran on the exchange stream
        last = max(i for i, r in enumerate(tr.trace[:opt_i]) if r.op == "launch" and r.b.startswith("c10d::"))
        at, _ = an.clocks()
        tl, pos, _ = at[last]
        assert at[opt_i][2].get(tl, 0) >= pos, "the optimizer is not ordered after the last exchange"
    assert all(all(x == x and abs(x) != float("inf") for x in step) for step in c["losses"]), c["losses"]
    if parity:
        want_l, want_g = _reference(golden_dir, compute, c["n"])
        assert c["losses"] == want_l, (c["losses"], want_l)
        g = c["grads"]
        assert torch.isfinite(g).all() and (g - want_g).abs().max() <= GRAD_TOL * want_g.abs().max(), \
            float((g - want_g).abs().max() / want_g.abs().max())


# ---------------------------------------------------------------------------------------------
# negative controls: edits of the recorded trace
# ---------------------------------------------------------------------------------------------
CONTROLS = [
    # case, function whose records are left out, kind of record, violation expected
    ("bf16", "_to_img", "wait", "conflict"),
    ("bf16", "_to_txt", "wait", "conflict"),
    # (in the device-input traces every tensor `_touch` names dies after `_to_txt` has joined the streams; the stager's tensors
    # come from the copy stream's pool, and the copy stream never waits for the image stream)
    ("host_stager", "_touch", "record_stream", "lifetime"),
    ("bf16_text_priority", "_on_text_stream", "wait", "conflict"),
    ("bf16_wgrad_stream", "_launch_wgrad", "wait", "conflict"),
    ("bf16_wgrad_stream", "_join_wgrad", "wait", "conflict"),
    ("bf16_wgrad_stream", "_launch_wgrad", "record_stream", "lifetime"),
    ("host_stager", "stage", "wait", "conflict"),
    ("dp", "_reduce_slice", "wait", "conflict"),
    ("dp", "_on_bucket", "wait", "conflict"),
]


@pytest.mark.parametrize("case,site,op,kind", CONTROLS)
def test_control_without_the_edges_of_one_site_the_checker_reports(case, site, op, kind, monkeypatch, golden_dir):
    c = _traced(case, monkeypatch, golden_dir)
    an = c["an"]
    drop = SO.from_site(an.trace, site, ops=(op,))
    assert drop, f"the {case} trace holds no {op} issued from {site}"
    found = [v for v in an.check(drop) if v.kind == kind]
    print(f"\n{case} without the {len(drop)} {op} records of {site}: {len(found)} {kind} violations")
    for v in found[:3]:
        print("   ", an.describe(v))
    assert found
