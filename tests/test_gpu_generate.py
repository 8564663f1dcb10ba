"""Answer generation on the GPU: the three new kernels against torch restatements, and generate_answers against the CPU oracle
(tiny config, teacher-forced), against sequence_log_likelihood of the completed sequences (full config), batch invariance and
no side effects."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_PATH = os.path.join(ROOT, "unimm_amd", "config", "bert_base_6layer_6conect.json")
SEP = 102


def relerr(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-6)).item()


# ---------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,beams", [(1, 1), (1, 16), (7, 4), (7, 16), (40, 1), (40, 4)])
@pytest.mark.parametrize("nr", [1, 2])
def test_attn_decode_matches_fp32_torch(G, beams, nr):
    from unimm_amd import lib as L
    g = torch.Generator().manual_seed(G * 100 + beams * 3 + nr)
    H, D, pcap = 12, 64, 20
    HD = H * D
    S = G * beams
    clen = torch.randint(1, 256, (G,), generator=g)
    clen[0] = 1
    clen[-1] = 255
    plen = torch.randint(0, pcap + 1, (S,), generator=g)
    plen[0], plen[-1] = 0, pcap
    coff = torch.cat([torch.zeros(1, dtype=torch.int64), clen.cumsum(0)[:-1]])
    ctx = (torch.randn(int(clen.sum()), 3 * HD, generator=g) * 1.5).to(torch.bfloat16)      # K | V columns at HD .. 3 HD
    priv = (torch.randn(S, pcap, 2 * HD, generator=g) * 1.5).to(torch.bfloat16)
    new = (torch.randn(S * nr, 3 * HD, generator=g) * 1.5).to(torch.bfloat16)
    sc = 1.0 / math.sqrt(D)
    dev = "cuda"
    ctx_d, priv_d, new_d = ctx.to(dev), priv.to(dev), new.to(dev)
    out = torch.zeros((S * nr, HD), dtype=torch.bfloat16, device=dev)
    pv = priv_d.view(S * pcap, 2 * HD)
    L.attn_decode(new_d[:, :HD], new_d[:, HD:2 * HD], new_d[:, 2 * HD:], out, ctx_d[:, HD:2 * HD], ctx_d[:, 2 * HD:],
                  coff.to(dev, torch.int32), clen.to(dev, torch.int32), pv[:, :HD], pv[:, HD:], plen.to(dev, torch.int32),
                  G, beams, nr, H, pcap, sc)
    torch.cuda.synchronize()
    want = torch.empty((S * nr, HD))
    f = lambda t: t.float()
    for s in range(S):
        gg = s // beams
        c0, c = int(coff[gg]), int(clen[gg])
        p = int(plen[s])
        for i in range(nr):
            r = s * nr + i
            k = torch.cat([f(ctx[c0:c0 + c, HD:2 * HD]), f(priv[s, :p, :HD]), f(new[s * nr:r + 1, HD:2 * HD])])
            v = torch.cat([f(ctx[c0:c0 + c, 2 * HD:]), f(priv[s, :p, HD:]), f(new[s * nr:r + 1, 2 * HD:])])
            q = f(new[r, :HD]).view(H, D)
            att = torch.softmax(torch.einsum("hd,khd->hk", q, k.view(-1, H, D)) * sc, -1)
            want[r] = torch.einsum("hk,khd->hd", att, v.view(-1, H, D)).reshape(HD)
    assert relerr(out.cpu(), want) < 2 ** -6, relerr(out.cpu(), want)


def test_attn_decode_equals_attn_fwd_shared_segment():
    """The same keys laid out for unimm_attn_fwd: the group's context as the shared segment (ks_*), private + new rows as the
    sequence's own keys, the generative mask as words.  Equal up to summation order."""
    from unimm_amd import lib as L
    g = torch.Generator().manual_seed(3)
    G, beams, nr, H, D, pcap = 5, 4, 2, 12, 64, 8
    HD, S = H * D, G * beams
    clen = torch.randint(1, 200, (G,), generator=g)
    plen = torch.randint(0, pcap + 1, (S,), generator=g)
    coff = torch.cat([torch.zeros(1, dtype=torch.int64), clen.cumsum(0)[:-1]])
    C = int(clen.sum())
    ctx = torch.randn(C, 3 * HD, generator=g).to(torch.bfloat16)
    priv = torch.randn(S, pcap, 2 * HD, generator=g).to(torch.bfloat16)
    new = torch.randn(S * nr, 3 * HD, generator=g).to(torch.bfloat16)
    dev = "cuda"
    sc = 1.0 / math.sqrt(D)
    out = torch.zeros((S * nr, HD), dtype=torch.bfloat16, device=dev)
    ctx_d, priv_d, new_d = ctx.to(dev), priv.to(dev), new.to(dev)
    pv = priv_d.view(S * pcap, 2 * HD)
    L.attn_decode(new_d[:, :HD], new_d[:, HD:2 * HD], new_d[:, 2 * HD:], out, ctx_d[:, HD:2 * HD], ctx_d[:, 2 * HD:],
                  coff.to(dev, torch.int32), clen.to(dev, torch.int32), pv[:, :HD], pv[:, HD:], plen.to(dev, torch.int32),
                  G, beams, nr, H, pcap, sc)
    # one packed row matrix: [context rows | per slot: private rows + new rows]; q rows are the new rows
    rows, k_off, k_len, q_off = [ctx], [], [], []
    base = C
    for s in range(S):
        p = int(plen[s])
        blk = torch.cat([torch.cat([torch.zeros(p, HD, dtype=torch.bfloat16), priv[s, :p]], 1), new[s * nr:(s + 1) * nr]])
        rows.append(blk)
        k_off.append(base)
        k_len.append(p + nr)
        q_off.append(base + p)
        base += p + nr
    X = torch.cat(rows).to(dev)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    Tk = 256
    nw = Tk // 32
    words = torch.zeros((S, 32, nw), dtype=torch.int64)
    for s in range(S):
        c, p = int(clen[s // beams]), int(plen[s])
        for i in range(nr):
            bits = torch.zeros(Tk, dtype=torch.int64)
            bits[:c + p + i + 1] = 1
            words[s, i] = (bits.view(nw, 32) << torch.arange(32)).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).to(dev)
    ref = torch.zeros((X.shape[0], HD), dtype=torch.bfloat16, device=dev)
    gidx = torch.arange(S) // beams
    L.attn_fwd(X[:, :HD], X[:, HD:2 * HD], X[:, 2 * HD:], ref, None, words, S, H, 32, Tk, D, sc, nw, 32 * nw, L.NO_DROP,
               qvar=(i32(q_off), i32([nr] * S)), kvar=(i32(k_off), i32(k_len)),
               kshared=(coff[gidx].to(dev, torch.int32), clen[gidx].to(dev, torch.int32), 0))
    torch.cuda.synchronize()
    qrows = torch.cat([torch.arange(o, o + nr) for o in q_off]).to(dev)
    assert relerr(out, ref[qrows]) < 1e-2, relerr(out, ref[qrows])


@pytest.mark.parametrize("V", [30522, 1000])
@pytest.mark.parametrize("K", [1, 4, 16])
def test_lm_topk_matches_float64(V, K):
    from unimm_amd import lib as L
    g = torch.Generator().manual_seed(V + K)
    rows = 24
    ld = (V + 63) // 64 * 64
    x = torch.randn(rows, ld, generator=g) * 3
    x[:, V:] = float("nan")                                       # padding columns are never read
    for r in range(rows):                                         # planted exact ties at the top
        top = int(torch.argmax(x[r, :V]))
        for j in torch.randint(0, V, (3,), generator=g).tolist():
            x[r, j] = x[r, top]
        x[r, (top + 7) % V] = x[r, (top + 11) % V] = x[r, top] - 0.5
    x[1, SEP] = 30.0                                              # SEP on top but banned on row 1
    x[2, SEP] = -50.0                                             # SEP forced on row 2
    x[4, 0] = 30.0                                                # a banned id on top
    flags = torch.zeros(rows, dtype=torch.int32)
    flags[1], flags[2], flags[3] = 1, 2, 3
    banned = [0, 101, 103]
    dev = "cuda"
    vals = torch.empty((rows, K), dtype=torch.float32, device=dev)
    ids = torch.empty((rows, K), dtype=torch.int32, device=dev)
    lse = torch.empty(rows, dtype=torch.float32, device=dev)
    L.lm_topk(x.to(dev), rows, V, torch.tensor(banned, dtype=torch.int32, device=dev), flags.to(dev), SEP, K, vals, ids, lse)
    torch.cuda.synchronize()
    lp = torch.log_softmax(x[:, :V].double(), -1)
    for r in range(rows):
        row = lp[r].clone()
        row[banned] = -math.inf
        if flags[r] & 1:
            row[SEP] = -math.inf
        if flags[r] & 2:
            keep = row[SEP].clone()
            row[:] = -math.inf
            row[SEP] = keep
        order = np.lexsort((np.arange(V), -row.numpy()))[:K]
        assert ids[r].cpu().tolist() == order.tolist(), (r, ids[r].cpu().tolist(), order.tolist())
        want = row[order].float()
        got = vals[r].cpu()
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got), fin)
        assert (got[fin] - want[fin]).abs().max().item() <= 1e-5 if fin.any() else True
    assert (lse.cpu().double() - torch.logsumexp(x[:, :V].double(), -1)).abs().max() < 1e-4


def test_kv_cache_update_bit_exact():
    from unimm_amd import lib as L
    g = torch.Generator().manual_seed(0)
    layers, slots, pcap, H, M = 12, 20, 6, 768, 40
    dev = "cuda"
    src = torch.randint(-30000, 30000, (layers, slots, pcap, 2 * H), generator=g, dtype=torch.int16).view(torch.bfloat16).to(dev)
    dst = torch.zeros_like(src)
    stash = torch.randint(-30000, 30000, (layers, M, 3 * H), generator=g, dtype=torch.int16).view(torch.bfloat16).to(dev)
    parent = torch.randint(0, slots, (slots,), generator=g).to(torch.int32)
    plen = torch.randint(0, pcap, (slots,), generator=g).to(torch.int32)
    plen_out = torch.full((slots,), -1, dtype=torch.int32, device=dev)
    L.kv_cache_update(src, dst, stash[0][:, H:], parent.to(dev), plen.to(dev), plen_out, layers, slots, pcap, 2 * H, M * 3 * H, 2)
    torch.cuda.synchronize()
    want = torch.zeros_like(src).cpu()
    s_c, st_c = src.cpu(), stash.cpu()
    for s in range(slots):
        p = int(parent[s])
        n = int(plen[p])
        want[:, s, :n] = s_c[:, p, :n]
        want[:, s, n] = st_c[:, 2 * p, H:]
    assert torch.equal(dst.cpu().view(torch.int16), want.view(torch.int16))
    assert plen_out.cpu().tolist() == (plen[parent.long()] + 1).tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
def make_dialogs(G, T, vocab, R, F, seed, cmin, cmax):
    """G dialog contexts laid out by oracle.masks.encode_gen (its context part), random images -> dict + the utterances."""
    from oracle import masks as OM
    rng = np.random.default_rng(seed)
    ids = np.zeros((G, T), dtype=np.int64)
    tt = np.zeros((G, T), dtype=np.int64)
    pp = np.zeros((G, T), dtype=np.int64)
    c = np.zeros(G, dtype=np.int64)
    utts = []
    for g in range(G):
        target = int(rng.integers(cmin, cmax + 1))
        u = []
        while 1 + sum(len(x) + 1 for x in u) < target - 3:
            u.append(rng.integers(1000 if vocab > 2000 else 110, vocab, int(rng.integers(1, 12))).tolist())
        u.append(rng.integers(110, vocab, 1).tolist())
        start = int(rng.integers(0, 2))
        enc = OM.encode_gen(u + [[]], start_segment=start, max_seq_len=T)
        cg = 1 + sum(len(x) + 1 for x in u)
        ids[g, :cg], tt[g, :cg], pp[g, :cg] = enc["tokens"][0, :cg], enc["segments"][0, :cg], enc["positions"][0, :cg]
        c[g] = cg
        utts.append((u, start))
    feat = torch.from_numpy(rng.standard_normal((G, R, F)).astype(np.float32))
    loc = torch.from_numpy(rng.random((G, R, 5)).astype(np.float32))
    T_ = torch.from_numpy
    return dict(input_ids=T_(ids), token_type_ids=T_(tt), position_ids=T_(pp), image_feat=feat, image_loc=loc,
                image_attention_mask=torch.ones((G, R), dtype=torch.int64)), c, utts


def completed(utts, answers, T):
    """encode_gen of every (dialog, answer) -> tensors of the completed sequences + copy-row offsets L."""
    from oracle import masks as OM
    out = {k: [] for k in ("tokens", "segments", "positions", "labels", "txt_attention_mask", "co_attention_mask")}
    Ls = []
    for (u, start), ans in zip(utts, answers):
        enc = OM.encode_gen(u + [list(ans)], start_segment=start, max_seq_len=T)
        for k in out:
            out[k].append(enc[k])
        Ls.append(1 + sum(len(x) + 1 for x in u) + len(ans) + 1)
    res = {k: torch.from_numpy(np.concatenate(v)) for k, v in out.items()}
    B, T_ = res["tokens"].shape
    res["co_attention_mask"] = res["co_attention_mask"][:, None, :].expand(B, 37, T_).contiguous()     # [B, R, T] (co-attention)
    return res, Ls


def answers_of(res, g, b):
    n = int(res.lengths[g, b])
    return res.tokens[g, b, :n - 1].tolist(), n


def gen_kwargs(d):
    return dict(token_type_ids=d["token_type_ids"], position_ids=d["position_ids"], image_attention_mask=d["image_attention_mask"])


@pytest.fixture(scope="module")
def tiny():
    from oracle import vilbert_ref as R
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    cfgd = json.load(open(os.path.join(ROOT, "tests", "golden", "small_config.json")))
    ocfg = R.make_config(cfgd)
    sd = R.init_state_dict(ocfg, seed=11)
    sd["cls.predictions.bias"] = torch.randn(sd["cls.predictions.bias"].shape, generator=torch.Generator().manual_seed(5)) * 3.0
    model = BertForMultiModalPreTraining(BertConfig.from_dict(cfgd))
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval(), ocfg, sd


def oracle_steps(ocfg, sd, d, idx, utts, answers, T):
    """Teacher-forced oracle: one forward of the completed sequences; copy row k = step k's distribution -> log p [B, steps, V]."""
    from oracle import vilbert_ref as R
    seq, Ls = completed([utts[i] for i in idx], answers, T)
    with torch.no_grad():
        out = R.forward(sd, ocfg, seq["tokens"], d["image_feat"][idx], d["image_loc"][idx], token_type_ids=seq["segments"],
                        position_ids=seq["positions"], attention_mask=seq["txt_attention_mask"],
                        image_attention_mask=d["image_attention_mask"][idx], co_attention_mask=seq["co_attention_mask"])
    lp = torch.log_softmax(out["pred_t"].double(), -1)
    return [lp[b, Ls[b]:Ls[b] + len(answers[b]) + 1] for b in range(len(idx))]


def banned_row(lp, k, limit, min_len=1):
    """The step-k rules (default banned ids, [SEP] banned before min_len, forced at the limit) on an oracle row of log p."""
    row = lp.clone()
    row[[0, 101, 103]] = -math.inf
    if k < min_len:
        row[SEP] = -math.inf
    if k >= limit:
        keep = row[SEP].clone()
        row[:] = -math.inf
        row[SEP] = keep
    return row


@pytest.mark.parametrize("beams", [1, 3])
def test_tiny_config_teacher_forced_against_oracle(tiny, beams):
    model, ocfg, sd = tiny
    T, G = 64, 6
    d, c, utts = make_dialogs(G, T, 1000, 37, 192, seed=beams, cmin=8, cmax=40)
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=beams, max_answer_len=8, **gen_kwargs(d))
    torch.cuda.synchronize()
    idx, answers, rows = [], [], []
    for g in range(G):
        for b in range(beams):
            ans, n = answers_of(res, g, b)
            assert n >= 2 and res.tokens[g, b, n - 1] == SEP and not set(ans) & {0, 101, 103, SEP}
            idx.append(g)
            answers.append(ans)
            rows.append((g, b, n))
    steps = oracle_steps(ocfg, sd, d, idx, utts, answers, T)
    clear = total = 0
    for (g, b, n), ans, lp in zip(rows, answers, steps):
        toks = ans + [SEP]
        want = torch.stack([lp[k, t] for k, t in enumerate(toks)])
        got = res.step_logp[g, b, :n].double().cpu()
        assert ((got - want).abs() <= 1e-2 + 1e-2 * want.abs()).all(), (g, b, got, want)
        assert abs(float(res.logp[g, b]) - float(want.sum())) <= 1e-2 * n + 1e-2 * abs(float(want.sum()))
        if beams == 1:
            for k, t in enumerate(toks):
                row = banned_row(lp[k], k, min(8, (T - int(c[g])) // 2 - 1))
                top2 = torch.topk(row, 2).values
                total += 1
                if float(top2[0] - top2[1]) > 0.05:
                    clear += 1
                    assert int(torch.argmax(row)) == t, (g, k)
    if beams == 1:
        print(f"\ngreedy: {clear} of {total} steps with an oracle top-2 margin above 0.05")
        assert clear >= 0.8 * total


def test_tiny_batch_invariance_and_no_side_effects(tiny):
    model, ocfg, sd = tiny
    T, G = 64, 80
    d, c, utts = make_dialogs(G, T, 1000, 37, 192, seed=9, cmin=8, cmax=40)
    seq, _ = completed(utts[:8], [[200, 300]] * 8, T)
    sargs = (seq["tokens"].cuda(), d["image_feat"][:8].cuda(), d["image_loc"][:8].cuda(), seq["labels"].cuda())
    skw = dict(token_type_ids=seq["segments"].cuda(), position_ids=seq["positions"].cuda(),
               attention_mask=seq["txt_attention_mask"].cuda(), co_attention_mask=seq["co_attention_mask"].cuda(),
               image_attention_mask=d["image_attention_mask"][:8].cuda())
    before, _ = model.sequence_log_likelihood(*sargs, **skw)
    batch = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=1, max_answer_len=10, **gen_kwargs(d))
    after, _ = model.sequence_log_likelihood(*sargs, **skw)
    torch.cuda.synchronize()
    assert torch.equal(before, after)
    answers = [answers_of(batch, g, 0)[0] for g in range(G)]
    steps = oracle_steps(ocfg, sd, d, list(range(G)), utts, answers, T)
    same = 0
    for g in (0, 17, 41, 79):
        sl = slice(g, g + 1)
        alone = model.generate_answers(d["input_ids"][sl], d["image_feat"][sl], d["image_loc"][sl], c[sl], beams=1,
                                       max_answer_len=10, **{k: v[sl] for k, v in gen_kwargs(d).items()})
        a, b = answers_of(alone, 0, 0)[0] + [SEP], answers[g] + [SEP]
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
        if k is None:
            assert a == b
            same += 1
            assert abs(float(alone.scores[0, 0]) - float(batch.scores[g, 0])) <= 1e-3 * abs(float(batch.scores[g, 0]))
        else:                                   # tokens may only differ where the oracle cannot separate the top two
            row = banned_row(steps[g][k], k, min(10, (T - int(c[g])) // 2 - 1))
            top2 = torch.topk(row, 2).values
            assert float(top2[0] - top2[1]) <= 0.05, (g, k)
    assert same >= 3


@pytest.fixture(scope="module")
def full():
    from oracle import vilbert_ref as R
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    model = BertForMultiModalPreTraining(BertConfig.from_json_file(CFG_PATH))
    ocfg = R.make_config(CFG_PATH)
    sd = R.init_state_dict(ocfg, seed=5)
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval(), ocfg, sd


@pytest.mark.parametrize("beams", [1, 4])
def test_full_config_scores_equal_sequence_log_likelihood(full, beams):
    model, ocfg, sd = full
    T, G = 256, 80
    d, c, utts = make_dialogs(G, T, 30522, 37, 2048, seed=100 + beams, cmin=10, cmax=200)
    for lpen in (0.0, 1.0):
        res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=beams, max_answer_len=20,
                                     length_penalty=lpen, **gen_kwargs(d))
        torch.cuda.synchronize()
        answers, gs = [], []
        for g in range(G):
            for b in range(beams):
                ans, n = answers_of(res, g, b)
                assert n >= 2 and res.tokens[g, b, n - 1] == SEP and not set(ans) & {0, 101, 103, SEP}
                answers.append(ans)
                gs.append(g)
        seq, _ = completed([utts[g] for g in gs], answers, T)
        dev = "cuda"
        want, _ = model.sequence_log_likelihood(seq["tokens"].to(dev), d["image_feat"][gs].to(dev), d["image_loc"][gs].to(dev),
                                                seq["labels"].to(dev), average=lpen == 1.0, token_type_ids=seq["segments"].to(dev),
                                                position_ids=seq["positions"].to(dev),
                                                attention_mask=seq["txt_attention_mask"].to(dev),
                                                co_attention_mask=seq["co_attention_mask"].to(dev),
                                                image_attention_mask=d["image_attention_mask"][gs].to(dev))
        got = res.scores.reshape(-1).cpu()
        want = want.cpu()
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        print(f"\nG = {G}, beams = {beams}, length_penalty = {lpen}: scores {float(got.min()):.3f} .. {float(got.max()):.3f}, "
              f"|generated - sequence_log_likelihood| {err:.3e} ({err / scale:.2e} of scale)")
        assert err <= 2e-3 * scale
        if lpen == 0.0:
            assert float((res.logp.reshape(-1).cpu() - want).abs().max()) <= 2e-3 * scale
            # two answers against the dense-logits oracle
            pick = [0, len(gs) - 1]
            steps = oracle_steps(ocfg, sd, d, [gs[i] for i in pick], utts, [answers[i] for i in pick], T)
            for i, lp in zip(pick, steps):
                g, b = divmod(i, beams)
                toks = answers[i] + [SEP]
                w = torch.stack([lp[k, t] for k, t in enumerate(toks)])
                gstep = res.step_logp[g, b, :len(toks)].double().cpu()
                assert (gstep - w).abs().max() <= 1e-2 * float(w.abs().max()), (gstep, w)
