"""The answer-generation kernels per element at every edge, against oracle/generate_ref.py (fp64 restatements of one launch
each; the budgets and their measured constants are derived there), and generate_answers where the dialogs of one batch have
different limits.

Every kernel case runs on buffers with guard rows before and after and a row stride wider than the payload; outputs are
pre-filled with a sentinel that everything outside the written region must keep, and every input element the contract says is
not read is NaN: the rows between the groups' contexts, private rows at and past plen[s], logits columns past V, cache columns
past `width`.  The gate is per element, |got - want| <= E; each family prints its worst |err| / E."""
import numpy as np
import pytest
import torch

from oracle import generate_ref as GR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
GUARD = GR.GUARD
SENT = -768.0                                   # exact in bf16 and fp32
SENT16 = 0x1234                                 # bit pattern the cache destinations start with
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------------------
# unimm_attn_decode
# ---------------------------------------------------------------------------------------------------------------------------
def launch_decode(case):
    """One launch on device copies of the case's buffers -> out [R, H D] float64; checks that nothing else was written."""
    from unimm_amd import lib as L
    HD, R = case["H"] * 64, case["R"]
    new, ctx = case["new"].to(DEV), case["ctx"].to(DEV)
    priv = case["priv"].to(DEV) if case["priv"] is not None else None
    outbuf = torch.full((GUARD + R + GUARD, HD + 8), SENT, dtype=BF16, device=DEV)
    out = outbuf[GUARD:GUARD + R, :HD]
    q, k, v, ck, cv, pk, pv = GR.decode_views(case, new, ctx, priv)
    i32 = lambda t: t.to(DEV, torch.int32)      # noqa: E731
    L.attn_decode(q, k, v, out, ck, cv, i32(case["ctx_off"]), i32(case["ctx_len"]), pk, pv, i32(case["plen"]), case["G"],
                  case["beams"], case["nr"], case["H"], case["pcap"], case["scale"])
    torch.cuda.synchronize()
    ob = outbuf.cpu().float()
    outside = torch.ones_like(ob, dtype=torch.bool)
    outside[GUARD:GUARD + R, :HD] = False
    assert (ob[outside] == SENT).all(), "attn_decode wrote outside out[:, :H * 64]"
    return ob[GUARD:GUARD + R, :HD].double()


def check_decode(case, what):
    got = launch_decode(case)
    ref = GR.attn_decode(*GR.decode_args(case, GR.decode_views(case)))
    assert torch.isfinite(ref["out"]).all()
    assert torch.isfinite(got).all(), (what, "a NaN: an input outside the key set was read")
    bad = (got - ref["out"]).abs() > ref["E"]
    if bad.any():
        r, col = [int(x) for x in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the budget, first (row {r}, col {col}, {int(ref['nk'][r])} keys): "
                             f"got {got[r, col]:.6f} want {ref['out'][r, col]:.6f} E {ref['E'][r, col]:.2e}")
    return GR.worst_ratio(got, ref["out"], ref["E"]), ref, got


@pytest.mark.parametrize("beams,nr", GR.DEC_BN)
@pytest.mark.parametrize("H", GR.DEC_H)
def test_attn_decode_edges(H, beams, nr):
    """G in {1, 3} x pcap in {0 (NULL private pointers), 1, 20, 62}; ctx_len from {0, 1, 7, 8, 9, 255, 256}, plen from
    {0, 1, 3, 4, 5, pcap, pcap + 2 (clamped), -1 (clamped)}; contexts with gaps and in reverse group order."""
    worst = 0.0
    for case in GR.decode_cross_cases(H, beams, nr):
        what = f"H {H} beams {beams} nr {nr} G {case['G']} pcap {case['pcap']} ctx_len {case['ctx_len'].tolist()}"
        worst = max(worst, check_decode(case, what)[0])
    print(f"\nattn_decode edges H = {H}, beams = {beams}, nr = {nr}: worst |err| / E = {worst:.3f}")


def test_attn_decode_documented_clamps():
    """plen > pcap behaves as pcap and negative plen as 0 (the same bits as the in-contract launch); ctx_len = 256, nr = 2,
    pcap = 64 sees 62 private rows (rows 62 and 63 are NaN here)."""
    w, ref, _ = check_decode(GR.truncation_case(), "ctx 256 + pcap 64")
    assert ref["nk"].tolist() == [319, 320] * 3
    a = GR.decode_case(3, 12, 4, 2, 1, 5, [7], [9, -3, 5, 0])
    b = dict(a, plen=torch.tensor([5, 0, 5, 0], dtype=torch.int32))
    wa, _, ga = check_decode(a, "plen [9, -3, 5, 0] of pcap 5")
    wb, _, gb = check_decode(b, "plen [5, 0, 5, 0] of pcap 5")
    assert torch.equal(ga, gb)
    print(f"\nattn_decode clamps: worst |err| / E = {max(w, wa, wb):.3f}")


def test_attn_decode_key_set_probes():
    """Every boundary of the key list: the chosen row's softmax sits on one chosen key, each V row carries its identity, and the
    real rows just outside the set would take all the mass if they were seen (oracle.generate_ref.probe_case)."""
    case = GR.probe_case()
    w, ref, got = check_decode(case, "probes")
    for qrow, h, vid in case["probes"]:
        lo, hi = float(got[qrow, h * 64]), float(got[qrow, h * 64 + 1])
        assert (round(lo), round(hi)) == (vid % 64, vid // 64), (qrow, h, vid, lo, hi)
    print(f"\nattn_decode probes ({len(case['probes'])}): worst |err| / E = {w:.3f}")


def test_cache_update_then_decode_chain():
    """The two kernels the way generation.py uses them: five steps of kv_cache_update on ping-pong buffers with random parents
    (the identity and `all children from one parent` among them), each followed by attn_decode on every layer; the oracle
    keeps every hypothesis's history as a Python list of rows."""
    from unimm_amd import lib as L
    g_ = torch.Generator().manual_seed(21)
    layers, G, beams, nr, pcap, H = 2, 2, 3, 2, 6, 2
    HD, S = H * 64, G * beams
    M, ldp, width = S * nr, 2 * H * 64 + 8, 2 * H * 64
    clen, coff = [9, 17], [20, 2]
    ctx = [GR._poisoned(40, 3 * HD) for _ in range(layers)]
    for c in ctx:
        for g in range(G):
            c[coff[g]:coff[g] + clen[g], HD:] = (torch.randn(clen[g], 2 * HD, generator=g_) * 1.5).to(BF16)
    ctx_d = [c.to(DEV) for c in ctx]
    priv = [torch.full((layers, S, pcap, ldp), float("nan"), dtype=BF16, device=DEV) for _ in range(2)]
    plen = [torch.zeros(S, dtype=torch.int32, device=DEV) for _ in range(2)]
    hist = [[] for _ in range(S)]                                   # per hypothesis: rows [layers, 2 H D]
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)  # noqa: E731
    stash = (torch.randn(layers, M, 3 * HD, generator=g_) * 1.5).to(BF16)
    grp = torch.arange(S) // beams * beams
    parents = [torch.arange(S), grp + 1, grp + torch.randint(0, beams, (S,), generator=g_),
               grp + torch.cat([torch.randperm(beams, generator=g_) for _ in range(G)]), grp + torch.randint(0, beams, (S,), generator=g_)]
    cur, worst = 0, 0.0
    for step, parent in enumerate(parents):
        stash_d = stash.to(DEV)
        L.kv_cache_update(priv[cur], priv[1 - cur], stash_d[0][:, HD:], parent.to(DEV, torch.int32), plen[cur], plen[1 - cur],
                          layers, S, pcap, width, M * 3 * HD, 2)
        cur = 1 - cur
        hist = [hist[int(p)] + [stash[:, 2 * int(p), HD:]] for p in parent]
        torch.cuda.synchronize()
        assert plen[cur].cpu().tolist() == [step + 1] * S
        want = torch.full((layers, S, pcap, ldp), float("nan"), dtype=BF16)
        for s in range(S):
            want[:, s, :step + 1, :width] = torch.stack(hist[s], 1)
        assert torch.equal(priv[cur].cpu().view(torch.int16), want.view(torch.int16)), f"cache after update {step}"
        stash = (torch.randn(layers, M, 3 * HD, generator=g_) * 1.5).to(BF16)
        stash_d = stash.to(DEV)
        for l in range(layers):
            out = torch.full((M, HD), SENT, dtype=BF16, device=DEV)
            pv = priv[cur][l].view(S * pcap, ldp)
            L.attn_decode(stash_d[l][:, :HD], stash_d[l][:, HD:2 * HD], stash_d[l][:, 2 * HD:], out, ctx_d[l][:, HD:2 * HD],
                          ctx_d[l][:, 2 * HD:], i32(coff), i32(clen), pv[:, :HD], pv[:, HD:2 * HD], plen[cur], G, beams, nr, H, pcap,
                          0.125)
            torch.cuda.synchronize()
            ph = want[l].reshape(S * pcap, ldp)
            ref = GR.attn_decode(stash[l][:, :HD], stash[l][:, HD:2 * HD], stash[l][:, 2 * HD:], ctx[l][:, HD:2 * HD], ctx[l][:, 2 * HD:],
                                 coff, clen, ph[:, :HD], ph[:, HD:2 * HD], [len(h) for h in hist], G, beams, nr, H, pcap, 0.125)
            got = out.cpu().double()
            assert torch.isfinite(got).all() and ((got - ref["out"]).abs() <= ref["E"]).all(), (step, l)
            worst = max(worst, GR.worst_ratio(got, ref["out"], ref["E"]))
    print(f"\ncache update + decode chain: worst |err| / E = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------
# unimm_lm_topk
# ---------------------------------------------------------------------------------------------------------------------------
def launch_topk(x, V, ld, banned, flags, K, rows=None):
    """-> (vals [rows, K], ids, lse) from guarded, sentinel-filled outputs; the logits buffer has NaN guard rows and columns."""
    from unimm_amd import lib as L
    n = x.shape[0]
    rows = n if rows is None else rows
    xb = torch.full((GUARD + n + GUARD, ld), float("nan"), dtype=torch.float32)
    xb[GUARD:GUARD + n, :V] = x
    xd = xb.to(DEV)
    vals = torch.full((GUARD + n + GUARD, K), SENT, dtype=torch.float32, device=DEV)
    ids = torch.full((GUARD + n + GUARD, K), -7, dtype=torch.int32, device=DEV)
    lse = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32, device=DEV)
    L.lm_topk(xd[GUARD:GUARD + n], rows, V, None if banned is None else banned.to(DEV), None if flags is None else flags.to(DEV),
              GR.TOPK_SEP, K, vals[GUARD:GUARD + n], ids[GUARD:GUARD + n], lse[GUARD:GUARD + n])
    torch.cuda.synchronize()
    vals, ids, lse = vals.cpu(), ids.cpu(), lse.cpu()
    body = slice(GUARD, GUARD + rows)
    keep = torch.ones(GUARD + n + GUARD, dtype=torch.bool)
    keep[body] = False
    assert (vals[keep] == SENT).all() and (ids[keep] == -7).all() and (lse[keep] == SENT).all(), "lm_topk wrote outside its rows"
    return vals[body], ids[body], lse[body]


@pytest.mark.parametrize("V", GR.TOPK_V)
def test_lm_topk_edges(V):
    """K in {1, 2, 15, 16} x (ldl padded, ldl == V) with the planted rows of oracle.generate_ref.topk_case, a banned list of 300
    ids (duplicates, negatives, ids >= V) and per-row flags; then flags = NULL and banned = NULL.  Ids exactly, finiteness
    exactly, values and lse within the budget."""
    tc = GR.topk_case(V)
    x, names = tc["x"], tc["names"]
    worst_v = worst_l = 0.0
    for banned, flags, lds in ((tc["banned"], tc["flags"], ((V + 63) // 64 * 64 + 64, V)), (None, None, (V,)),
                               (tc["banned"], None, (V + 1,)), (None, tc["flags"], (V,))):
        ref = GR.lm_topk(x, V, banned, flags, GR.TOPK_SEP, 16)
        for ld in lds:
            for K in GR.TOPK_K:
                vals, ids, lse = launch_topk(x, V, ld, banned, flags, K)
                what = f"V {V} K {K} ldl {ld} banned {banned is not None} flags {flags is not None}"
                for r in range(x.shape[0]):
                    assert ids[r].tolist() == ref["ids"][r, :K].tolist(), (what, names[r], ids[r].tolist(), ref["ids"][r, :K].tolist())
                want, E = ref["vals"][:, :K], ref["E_val"][:, :K]
                fin = torch.isfinite(want)
                assert torch.equal(torch.isfinite(vals), fin) and not torch.isnan(vals).any(), what
                err = torch.where(fin, (vals.double() - want).abs(), torch.zeros_like(want))
                assert (err <= E).all(), (what, names[int((err / E).max(1).values.argmax())], float((err / E).max()))
                el = (lse.double() - ref["lse"]).abs()
                assert (el <= ref["E_lse"]).all(), (what, names[int((el / ref["E_lse"]).argmax())], float((el / ref["E_lse"]).max()))
                worst_v, worst_l = max(worst_v, float((err / E).max())), max(worst_l, float((el / ref["E_lse"]).max()))
    print(f"\nlm_topk V = {V}: worst |err| / E: vals {worst_v:.3f}, lse {worst_l:.3f}")


def test_lm_topk_zero_rows_and_no_lse():
    from unimm_amd import lib as L
    V, K = 257, 4
    tc = GR.topk_case(V)
    vals, ids, lse = launch_topk(tc["x"], V, V, tc["banned"], tc["flags"], K, rows=0)      # everything keeps the sentinel
    assert vals.numel() == 0
    x = tc["x"].to(DEV)
    v = torch.full((x.shape[0], K), SENT, dtype=torch.float32, device=DEV)
    i = torch.full((x.shape[0], K), -7, dtype=torch.int32, device=DEV)
    L.lm_topk(x, x.shape[0], V, None, None, GR.TOPK_SEP, K, v, i, None)                      # lse = NULL
    torch.cuda.synchronize()
    ref = GR.lm_topk(tc["x"], V, None, None, GR.TOPK_SEP, K)
    assert torch.equal(i.cpu().long(), ref["ids"])
    assert ((v.cpu().double() - ref["vals"]).abs() <= ref["E_val"]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# unimm_kv_cache_update
# ---------------------------------------------------------------------------------------------------------------------------
KV_CASES = [  # layers, slots, pcap, width, new_row_mul, parent
    (1, 1, 1, 8, 1, "identity"), (1, 20, 2, 8, 2, "constant"), (12, 20, 20, 1536, 2, "permutation"), (12, 300, 2, 1536, 1, "out of range"),
    (1, 300, 20, 1536, 2, "random"), (12, 1, 20, 8, 1, "identity"), (1, 20, 1, 1536, 1, "out of range"), (12, 300, 1, 8, 2, "permutation"),
    (1, 1, 2, 1536, 2, "out of range"), (12, 20, 2, 8, 1, "random"), (1, 20, 20, 8, 2, "permutation"), (12, 20, 20, 8, 1, "constant"),
]


def kv_case(layers, slots, pcap, width, row_mul, mode, seed):
    g_ = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randint(-30000, 30000, shape, generator=g_, dtype=torch.int16).view(BF16)      # noqa: E731
    ldp, ld_new = width + 8, width + 24
    plen = torch.randint(0, pcap + 1, (slots,), generator=g_)
    for i, val in enumerate((0, pcap - 1, pcap, -2)):              # pcap and -2 are out of contract: clamped
        if i < slots:
            plen[(7 * i) % slots] = val
    parent = dict(identity=torch.arange(slots), constant=torch.full((slots,), slots // 2),
                  permutation=torch.randperm(slots, generator=g_), random=torch.randint(0, slots, (slots,), generator=g_))
    parent["out of range"] = torch.randint(-3, slots + 3, (slots,), generator=g_)
    parent["out of range"][0], parent["out of range"][-1] = -1, slots + 5
    src = torch.full((layers, slots, pcap, ldp), float("nan"), dtype=BF16)
    for s in range(slots):
        n = min(max(int(plen[s]), 0), pcap - 1)
        src[:, s, :n, :width] = rnd(layers, n, width)               # rows at and past plen and columns past width: never read
    rows_l = slots * row_mul + 3                                    # a layer's new rows + 3 rows nobody owns
    stash = torch.full((layers, rows_l, ld_new), float("nan"), dtype=BF16)
    stash[:, 0:slots * row_mul:row_mul, 8:8 + width] = rnd(layers, slots, width)
    return dict(src=src, stash=stash, parent=parent[mode].to(torch.int32), plen=plen.to(torch.int32), ldp=ldp, nls=rows_l * ld_new)


@pytest.mark.parametrize("layers,slots,pcap,width,row_mul,mode", KV_CASES)
def test_kv_cache_update_edges(layers, slots, pcap, width, row_mul, mode):
    from unimm_amd import lib as L
    c = kv_case(layers, slots, pcap, width, row_mul, mode, seed=layers + slots + pcap + width)
    ldp = c["ldp"]
    n = layers * slots * pcap
    dbuf = torch.full((GUARD + n + GUARD, ldp), SENT16, dtype=torch.int16).view(BF16)
    dst_h = dbuf[GUARD:GUARD + n].view(layers, slots, pcap, ldp)
    want, plen_out = GR.kv_cache_update(c["src"], dst_h, c["stash"][0][:, 8:], c["parent"], c["plen"], layers, slots, pcap, width,
                                        c["nls"], row_mul)
    dbuf_d = dbuf.clone().to(DEV)
    dst_d = dbuf_d[GUARD:GUARD + n].view(layers, slots, pcap, ldp)
    stash_d = c["stash"].to(DEV)
    po = torch.full((GUARD + slots + GUARD,), -7, dtype=torch.int32, device=DEV)
    L.kv_cache_update(c["src"].to(DEV), dst_d, stash_d[0][:, 8:], c["parent"].to(DEV), c["plen"].to(DEV), po[GUARD:GUARD + slots],
                      layers, slots, pcap, width, c["nls"], row_mul)
    torch.cuda.synchronize()
    got = dbuf_d.cpu().view(torch.int16)
    assert (got[:GUARD] == SENT16).all() and (got[GUARD + n:] == SENT16).all(), "guard rows"
    got = got[GUARD:GUARD + n].view(layers, slots, pcap, ldp)
    assert torch.equal(got, want.view(torch.int16)), f"{int((got != want.view(torch.int16)).sum())} elements differ"
    assert (got[..., :width] != 0x7FC0).all()                        # the NaN of the unread rows was copied nowhere
    po = po.cpu()
    assert po[GUARD:GUARD + slots].tolist() == plen_out.tolist() and (po[:GUARD] == -7).all() and (po[GUARD + slots:] == -7).all()


def test_kv_cache_update_error_codes():
    """src == dst, plen == plen_out and misaligned arguments are refused before any launch: dst keeps its contents."""
    from unimm_amd import lib as L
    layers, slots, pcap, width = 2, 4, 3, 16
    src = torch.zeros((layers, slots, pcap, width + 8), dtype=BF16, device=DEV)
    dst = torch.full_like(src, SENT)
    stash = torch.zeros((layers, slots, width + 8), dtype=BF16, device=DEV)
    parent = torch.arange(slots, dtype=torch.int32, device=DEV)
    plen = torch.zeros(slots, dtype=torch.int32, device=DEV)
    po = torch.full((slots,), -7, dtype=torch.int32, device=DEV)
    nls = slots * (width + 8)
    call = lambda s, d, nk, pl, pout, w: L.kv_cache_update(s, d, nk, parent, pl, pout, layers, slots, pcap, w, nls, 1)   # noqa: E731
    with pytest.raises(L.UnimmHipError, match="UNIMM_E_ARG"):
        call(src, src, stash[0], plen, po, width)
    with pytest.raises(L.UnimmHipError, match="UNIMM_E_ARG"):
        call(src, dst, stash[0], plen, plen, width)
    with pytest.raises(L.UnimmHipError, match="UNIMM_E_ALIGN"):
        call(src, dst, stash[0][:, 4:], plen, po, width)             # new_kv 8 bytes off
    with pytest.raises(L.UnimmHipError, match="UNIMM_E_ALIGN"):
        call(src, dst, stash[0], plen, po, 12)                       # width % 8
    with pytest.raises(L.UnimmHipError, match="UNIMM_E_SHAPE"):
        call(src, dst, stash[0], plen, po, width + 16)               # width > ldp
    torch.cuda.synchronize()
    assert (dst.float() == SENT).all() and (po == -7).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the model: per-dialog limits that differ inside one batch
# ---------------------------------------------------------------------------------------------------------------------------
from tests.test_gpu_generate import SEP, answers_of, banned_row, completed, gen_kwargs, oracle_steps, tiny  # noqa: E402,F401

T, MAXLEN, R_IMG, FEAT = 64, 8, 37, 192


def exact_dialogs(cs, seed, vocab=1000):
    """Dialog contexts of EXACTLY cs[g] tokens, laid out by oracle.masks.encode_gen -> (inputs, c, utterances) as
    tests.test_gpu_generate.make_dialogs returns them."""
    from oracle import masks as OM
    rng = np.random.default_rng(seed)
    G = len(cs)
    ids, tt, pp = (np.zeros((G, T), dtype=np.int64) for _ in range(3))
    utts = []
    for g, c in enumerate(cs):
        left, u = c - 1, []                                          # an utterance of n tokens takes n + 1 positions
        while left:
            n = int(rng.integers(1, 12))
            n = min(n, left - 1)
            if left - 1 - n == 1:
                n = n - 1 if n > 1 else n + 1
            u.append(rng.integers(110, vocab, n).tolist())
            left -= n + 1
        start = int(rng.integers(0, 2))
        enc = OM.encode_gen(u + [[]], start_segment=start, max_seq_len=T)
        assert 1 + sum(len(x) + 1 for x in u) == c
        ids[g, :c], tt[g, :c], pp[g, :c] = enc["tokens"][0, :c], enc["segments"][0, :c], enc["positions"][0, :c]
        utts.append((u, start))
    feat = torch.from_numpy(rng.standard_normal((G, R_IMG, FEAT)).astype(np.float32))
    loc = torch.from_numpy(rng.random((G, R_IMG, 5)).astype(np.float32))
    F = torch.from_numpy
    return dict(input_ids=F(ids), token_type_ids=F(tt), position_ids=F(pp), image_feat=feat, image_loc=loc,
                image_attention_mask=torch.ones((G, R_IMG), dtype=torch.int64)), np.asarray(cs, dtype=np.int64), utts


def check_generation(model, ocfg, sd, d, c, utts, res, beams, min_len, greedy_stats=None):
    """The assertions of the issue on one generate_answers result (length_penalty 0)."""
    G = len(c)
    limits = np.minimum(MAXLEN, (T - c) // 2 - 1)
    idx, answers, rows = [], [], []
    for g in range(G):
        nfin = 0
        for b in range(beams):
            n = int(res.lengths[g, b])
            if n == 0:                                               # padding of a dialog that finished fewer than `beams`
                assert not res.tokens[g, b].any() and res.scores[g, b] == -float("inf") and res.logp[g, b] == -float("inf"), (g, b)
                assert not (res.lengths[g, b:] != 0).any(), "padding comes last"
                continue
            nfin += 1
            ans = res.tokens[g, b, :n - 1].tolist()
            assert res.tokens[g, b, n - 1] == SEP and not set(ans) & {0, 101, 103, SEP} and not res.tokens[g, b, n:].any()
            assert min_len <= len(ans) <= limits[g], (g, b, len(ans), int(limits[g]))
            idx.append(g)
            answers.append(ans)
            rows.append((g, b, n))
        assert nfin >= 1
        if limits[g] == 0:
            assert nfin == 1 and int(res.lengths[g, 0]) == 1         # [SEP] was forced at step 0: one hypothesis, the rest padding
    steps = oracle_steps(ocfg, sd, d, idx, utts, answers, T)
    for (g, b, n), ans, lp in zip(rows, answers, steps):
        toks = ans + [SEP]
        want = torch.stack([lp[k, t] for k, t in enumerate(toks)])
        got = res.step_logp[g, b, :n].double().cpu()
        assert ((got - want).abs() <= 1e-2 + 1e-2 * want.abs()).all(), (g, b, got, want)
        if greedy_stats is not None:
            for k, t in enumerate(toks):
                row = banned_row(lp[k], k, int(limits[g]), min_len)
                top2 = torch.topk(row, 2).values
                greedy_stats[1] += 1
                if float(top2[0] - top2[1]) > 0.05:
                    greedy_stats[0] += 1
                    assert int(torch.argmax(row)) == t, (g, k)
    # scores = sequence_log_likelihood of the completed sequences
    seq, _ = completed([utts[g] for g in idx], answers, T)
    want, _ = model.sequence_log_likelihood(seq["tokens"].to(DEV), d["image_feat"][idx].to(DEV), d["image_loc"][idx].to(DEV),
                                            seq["labels"].to(DEV), average=False, token_type_ids=seq["segments"].to(DEV),
                                            position_ids=seq["positions"].to(DEV), attention_mask=seq["txt_attention_mask"].to(DEV),
                                            co_attention_mask=seq["co_attention_mask"].to(DEV),
                                            image_attention_mask=d["image_attention_mask"][idx].to(DEV))
    want = want.cpu()
    got = torch.stack([res.scores[g, b] for g, b, _ in rows]).cpu()
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= 2e-3 * scale, (err, scale)
    return err / scale


# context lengths -> limits min(8, (64 - c) // 2 - 1): {0, 1, 2, 5, 8, 0, 8} for min_answer_len 0, {3, 4, 5, 8, 3, 8} for 3
LIMIT_CONTEXTS = {0: [62, 60, 58, 52, 30, 61, 12], 3: [56, 54, 52, 30, 55, 12]}


@pytest.mark.parametrize("min_len", [0, 3])
@pytest.mark.parametrize("beams", [1, 4, 16])
def test_tiny_config_mixed_limits(tiny, beams, min_len):
    """One batch whose dialogs have the limits {0, 1, 2, 5, max_answer_len} (min_answer_len 0; c = T - 2 forces [SEP] at step 0)
    or {3, 4, 5, max_answer_len} (min_answer_len 3): SEP_FORCED differs between the rows of one step, dialogs stop while others
    go on, and a dialog of limit 0 finishes one hypothesis only."""
    model, ocfg, sd = tiny
    cs = LIMIT_CONTEXTS[min_len]
    d, c, utts = exact_dialogs(cs, seed=50 + min_len)
    lim = np.minimum(MAXLEN, (T - c) // 2 - 1).tolist()
    assert sorted(set(lim)) == ([0, 1, 2, 5, 8] if min_len == 0 else [3, 4, 5, 8])
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=beams, max_answer_len=MAXLEN,
                                 min_answer_len=min_len, **gen_kwargs(d))
    torch.cuda.synchronize()
    stats = [0, 0] if beams == 1 else None
    rel = check_generation(model, ocfg, sd, d, c, utts, res, beams, min_len, stats)
    print(f"\nmixed limits {lim}, beams {beams}, min_answer_len {min_len}: |scores - sequence_log_likelihood| {rel:.2e} of scale")
    if stats is not None:
        print(f"greedy: {stats[0]} of {stats[1]} steps with an oracle top-2 margin above 0.05")
        assert stats[0] >= 0.8 * stats[1]


def test_tiny_config_image_index_equals_repeated_images(tiny):
    model, ocfg, sd = tiny
    d, c, utts = exact_dialogs([30, 58, 41, 62, 20, 52], seed=7)
    index = torch.tensor([0, 0, 1, 0, 1, 2])
    feat, loc = d["image_feat"][:3], d["image_loc"][:3]
    kw = dict(beams=4, max_answer_len=MAXLEN, min_answer_len=0, **gen_kwargs(d))
    shared = model.generate_answers(d["input_ids"], feat, loc, c, image_index=index, **kw)
    d["image_feat"], d["image_loc"] = feat[index], loc[index]
    rep = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, **kw)
    torch.cuda.synchronize()
    for name in ("tokens", "lengths", "scores", "logp", "step_logp"):
        assert torch.equal(getattr(shared, name), getattr(rep, name)), name
    check_generation(model, ocfg, sd, d, c, utts, rep, 4, 0)


def test_tiny_config_one_dialog_one_beam(tiny):
    """G = 1, beams = 1: two decode rows per step."""
    model, ocfg, sd = tiny
    d, c, utts = exact_dialogs([23], seed=3)
    res = model.generate_answers(d["input_ids"], d["image_feat"], d["image_loc"], c, beams=1, max_answer_len=MAXLEN,
                                 min_answer_len=3, **gen_kwargs(d))
    torch.cuda.synchronize()
    assert int(res.lengths[0, 0]) >= 4
    check_generation(model, ocfg, sd, d, c, utts, res, 1, 3)
