"""What the CIDEr-D reward costs (include/unimm_reward.h; unimm_amd/reward.py), at G = 80 dialogs x N = 8 samples against M = 100
references in 21-token rows (answers of 1 .. 20 tokens and their [SEP], ids of the 30522-word vocabulary; a hypothesis copies
about two thirds of a reference of its dialog, so that every order has matches):

  (a) kernel   the `unimm_ngram_reward` launch, uniform weights (all 100 references walked), with a document-frequency table of
               the references and without one: device time between two events around `--launches` back-to-back launches.
  (b) host     tests/reward_ref.py, the float64 restatement in Python dicts, on the same inputs: one pass by the host clock.
  (c) step     the 8 x 8 fused-rollout `trainer.self_critical_step` of tools/bench_policy.py (full configuration, temperature
               0.8 / top-k 50 / top-p 0.9) with `CiderD` as the reward, against the same step with a host callable that returns
               zeros -- the step as it is without the feature, with a reward that costs nothing.  Two warm-up steps of each, then
               `--pairs` alternating pairs by the host clock.  The condition: the median with CiderD is not above the median with
               the zero reward by more than the zero-reward step's own min-to-max spread.

    python tools/bench_reward.py [--part kernel,host,step] [--pairs 7] [--launches 50]

prints what it measures and ends with one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG_PATH = os.path.join(ROOT, "unimm_amd", "config", "bert_base_6layer_6conect.json")
SEP, VOCAB, W = 102, 30522, 21


def answers(G, N, M, seed):
    """(hyp [G, N, W], hyp_len [G, N], ref [G, M, W], ref_len [G, M]) int64 on the host"""
    rng = np.random.default_rng(seed)

    def rows(shape, L):
        t = rng.integers(1000, VOCAB, size=shape + (W,))
        pos = np.arange(W)
        t = np.where(pos < L[..., None], t, 0)
        return np.where(pos == L[..., None], SEP, t)

    ref_L = rng.integers(1, W, size=(G, M))
    ref = rows((G, M), ref_L)
    hyp_L = rng.integers(1, W, size=(G, N))
    hyp = rows((G, N), hyp_L)
    src = ref[np.arange(G)[:, None], rng.integers(0, M, size=(G, N))]                       # [G, N, W]
    cyc = np.stack([np.resize(src[g, i, :max(1, int((src[g, i] == SEP).argmax()))], W) for g in range(G) for i in range(N)])
    take = (rng.random((G, N, W)) < 0.67) & (np.arange(W) < hyp_L[..., None])
    hyp = np.where(take, cyc.reshape(G, N, W), hyp)
    T = torch.from_numpy
    return T(hyp), T(hyp_L + 1), T(ref), T(ref_L + 1)


def kernel(G, N, M, launches):
    from unimm_amd import reward
    hyp, hl, ref, rl = answers(G, N, M, seed=1)
    table = reward.NgramTable.from_corpus(ref.reshape(-1, W), rl.reshape(-1))
    dev = dict(hyp=hyp.cuda(), hl=hl.cuda(), ref=ref.cuda(), rl=rl.cuda())
    out = {}
    for name, tab in (("table", table), ("no_table", None)):
        scorer = reward.CiderD(tab)
        from unimm_amd import reward_abi as A
        h32, l32 = dev["hyp"].reshape(G * N, W).int(), dev["hl"].reshape(-1).int()
        g32 = torch.arange(G, dtype=torch.int32, device="cuda").repeat_interleave(N)
        r32, rl32 = dev["ref"].int(), dev["rl"].int()
        res = torch.empty(G * N, dtype=torch.float32, device="cuda")

        def go():
            A.ngram_reward(h32, l32, g32, r32, rl32, None, None if tab is None else tab.keys, None if tab is None else tab.idf,
                           0.0 if tab is None else tab.default_idf, 6.0, res)
        for _ in range(3):
            go()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                go()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / launches)
        t0 = time.perf_counter()
        full = scorer.score(dev["hyp"], dev["hl"], dev["ref"], dev["rl"])                  # the surface: checks, staging, launch
        host_view = full.cpu()
        surface_ms = (time.perf_counter() - t0) * 1e3
        assert torch.equal(host_view.reshape(-1), res.cpu())
        out[name] = dict(launch_us=round(statistics.median(times), 1), launch_us_min_max=[round(min(times), 1), round(max(times), 1)],
                         score_call_to_host_ms=round(surface_ms, 3), mean_reward=round(float(host_view.mean()), 4),
                         table_slots=None if tab is None else tab.cap)
        print(f"unimm_ngram_reward (S = {G * N}, M = {M}, {name}): {out[name]}")
    return out


def host(G, N, M):
    sys.path.insert(0, ROOT)
    from tests import reward_ref as RR
    from unimm_amd import reward
    hyp, hl, ref, rl = answers(G, N, M, seed=1)
    out = {}
    for name in ("table", "no_table"):
        t0 = time.perf_counter()
        idf = RR.corpus_idf(ref.reshape(-1, W).tolist(), rl.reshape(-1).tolist()) if name == "table" else RR.unit_idf
        t1 = time.perf_counter()
        want = RR.score(hyp.tolist(), hl.tolist(), ref.tolist(), rl.tolist(), None, idf)
        t2 = time.perf_counter()
        out[name] = dict(score_s=round(t2 - t1, 3), corpus_s=round(t1 - t0, 3), mean_reward=round(float(want.mean()), 4))
        if torch.cuda.is_available():
            tab = reward.NgramTable.from_corpus(ref.reshape(-1, W), rl.reshape(-1)) if name == "table" else None
            got = reward.CiderD(tab).score(hyp, hl, ref, rl).cpu().numpy()
            out[name]["max_abs_difference_from_device"] = float(np.abs(got - want.astype(np.float32)).max())
        print(f"tests/reward_ref.py on the host (S = {G * N}, M = {M}, {name}): {out[name]}")
    return out


def step(pairs, M):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_generate import dialogs
    from oracle import vilbert_ref as RF
    from unimm_amd import VisualDialogEncoder, policy, reward, trainer
    from unimm_amd.optim import FusedAdamW, WarmupLinearScheduleNonZero, default_language_weights, reference_param_groups
    G = N = 8
    enc = VisualDialogEncoder(CFG_PATH)
    enc.bert_pretrained.load_state_dict(RF.init_state_dict(RF.make_config(CFG_PATH), seed=5), strict=True)
    enc = enc.cuda()
    groups = reference_param_groups(enc, lr=1e-5, image_lr=1e-5, language_weights=default_language_weights(enc))
    opt = FusedAdamW(groups, enc.bert_pretrained.engine, lr=1e-5)
    sch = WarmupLinearScheduleNonZero(opt, warmup_steps=2, t_total=100, min_lr=1e-6)
    d, c = dialogs(G, seed=3)
    _, _, ref, rl = answers(G, N, M, seed=2)
    batch = dict(tokens=d["input_ids"], segments=d["token_type_ids"], positions=d["position_ids"], context_len=c,
                 image_feat=d["image_feat"], image_loc=d["image_loc"], image_mask=d["image_attention_mask"],
                 reference_tokens=ref.cuda(), reference_lengths=rl.cuda())
    table = reward.NgramTable.from_corpus(ref.reshape(-1, W), rl.reshape(-1))
    forms = {"zero": lambda tokens, lengths: torch.zeros(lengths.shape), "cider_d": reward.CiderD(table)}
    it = 0

    def one(form, seed):
        nonlocal it
        it += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = trainer.self_critical_step(enc, opt, sch, batch, dict(batch_multiply=1), it, forms[form], samples=N, baseline="greedy",
                                         objective=policy.PolicyObjective(entropy_coef=0.01), temperature=0.8, top_k=50, top_p=0.9,
                                         seed=seed, rollout="fused")
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        print(f"self_critical_step {it} ({form}): {ms:.2f} ms, loss {out[0]:.6f}, reward {out[1]:.4f}")
        return ms

    for _ in range(2):
        for form in forms:
            one(form, 0)
    t = {form: [] for form in forms}
    for pair in range(1, pairs + 1):
        for form in forms:
            t[form].append(one(form, pair))
    med = {f: statistics.median(v) for f, v in t.items()}
    spread = max(t["zero"]) - min(t["zero"])
    res = dict(G=G, N=N, M=M, pairs=pairs, median_ms={f: round(v, 2) for f, v in med.items()},
               ms={f: [round(x, 2) for x in v] for f, v in t.items()}, zero_spread_ms=round(spread, 2),
               extra_ms=round(med["cider_d"] - med["zero"], 2), within_zero_spread=bool(med["cider_d"] - med["zero"] <= spread))
    print(f"8 x 8 fused-rollout step, CiderD against a zero host reward: {res}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernel,host,step")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    parts, out = a.part.split(","), {}
    if "kernel" in parts:
        out["kernel"] = kernel(80, 8, 100, a.launches)
    if "host" in parts:
        out["host"] = host(80, 8, 100)
    if "step" in parts:
        out["step"] = step(a.pairs, 100)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
