"""oracle/generate_ref.py against independent statements of the same operations, on the CPU: the decode restatement against
oracle.attention_ref given the same rows as one packed launch with the generative mask words, the top-K restatement against
torch.topk / a brute-force sort, the float32 restatements against the budgets with the recorded constants, and a chain of
kv_cache_update restatements against per-hypothesis Python lists."""
import math

import numpy as np
import pytest
import torch

from oracle import attention_ref as AR
from oracle import generate_ref as GR

BF16 = torch.bfloat16


def test_decode_equals_attention_ref_with_generative_mask_words():
    """The header's claim that the key list needs no mask words, in fp64: the group's context as the shared segment, private +
    new rows as the slot's own keys, bit (i, j) set for j < c + plen + i + 1 (test_attn_decode_equals_attn_fwd_shared_segment
    lays a launch out the same way)."""
    G, beams, nr, H, pcap = 3, 3, 2, 2, 8
    HD, S = H * 64, G * beams
    case = GR.decode_case(5, H, beams, nr, G, pcap, [9, 40, 0], [0, 1, 8, 3, 4, 5, 8, 2, 0])
    views = GR.decode_views(case)
    q, k, v, ck, cv, pk, pv = views
    ref = GR.attn_decode(*GR.decode_args(case, views))
    ctx, plen, clen, coff = case["ctx"], case["plen"].tolist(), case["ctx_len"].tolist(), case["ctx_off"].tolist()
    rows, k_off, k_len, q_off = [ctx], [], [], []
    base = ctx.shape[0]
    for s in range(S):
        p = plen[s]
        own = torch.cat([q[s * nr:(s + 1) * nr], k[s * nr:(s + 1) * nr], v[s * nr:(s + 1) * nr]], 1)
        rows.append(torch.cat([torch.cat([torch.zeros(p, HD, dtype=BF16), pk[s * pcap:s * pcap + p], pv[s * pcap:s * pcap + p]], 1), own]))
        k_off.append(base)
        k_len.append(p + nr)
        q_off.append(base + p)
        base += p + nr
    X = torch.cat(rows)
    Tk = 64
    bits = np.zeros((S, nr, Tk), dtype=bool)
    for s in range(S):
        for i in range(nr):
            bits[s, i, :clen[s // beams] + plen[s] + i + 1] = True
    words = AR.pack_bits(bits)
    nw = Tk // 32
    gi = [s // beams for s in range(S)]
    res = AR.attention(X[:, :HD], X[:, HD:2 * HD], X[:, 2 * HD:], words, B=S, H=H, Tq=nr, Tk=Tk, D=64, scale=case["scale"],
                       mask_q_stride=nw, mask_b_stride=nr * nw, qvar=(q_off, [nr] * S), kvar=(k_off, k_len),
                       kshared=([coff[g] for g in gi], [clen[g] for g in gi], 0))
    qrows = torch.cat([torch.arange(o, o + nr) for o in q_off])
    want = res["out"][qrows]
    assert torch.isfinite(ref["out"]).all()
    assert (ref["out"] - want).abs().max() <= 1e-12 * want.abs().max()
    assert ref["nk"].tolist() == [clen[s // beams] + plen[s] + i + 1 for s in range(S) for i in range(nr)]


def test_decode_clamps_and_probes():
    """plen > pcap behaves as pcap, negative as 0, and ctx 256 + nr 2 truncates to 62 private rows; every probe's wanted output
    decodes to the identity of the chosen V row."""
    case = GR.truncation_case()
    ref = GR.attn_decode(*GR.decode_args(case, GR.decode_views(case)))
    assert ref["nk"].tolist() == [256 + 62 + 1, 256 + 62 + 2] * 3 and torch.isfinite(ref["out"]).all()
    a = GR.decode_case(3, 1, 4, 2, 1, 5, [7], [9, -3, 5, 0])
    b = dict(a, plen=torch.tensor([5, 0, 5, 0], dtype=torch.int32))
    ra, rb = (GR.attn_decode(*GR.decode_args(c, GR.decode_views(c))) for c in (a, b))
    assert torch.equal(ra["out"], rb["out"]) and torch.isfinite(ra["out"]).all()
    case = GR.probe_case()
    ref = GR.attn_decode(*GR.decode_args(case, GR.decode_views(case)))
    assert torch.isfinite(ref["out"]).all() and len(case["probes"]) == 18
    for qrow, h, vid in case["probes"]:
        lo, hi = ref["out"][qrow, h * 64].item(), ref["out"][qrow, h * 64 + 1].item()
        assert abs(lo - vid % 64) < 1e-6 and abs(hi - vid // 64) < 1e-6, (qrow, h, vid, lo, hi)


def test_topk_against_torch_and_brute_force():
    V, K = 1000, 16
    tc = GR.topk_case(V)
    x, names = tc["x"], tc["names"]
    plain = GR.lm_topk(x, V, None, None, GR.TOPK_SEP, K)
    lp = torch.log_softmax(x.double(), -1)
    r = names.index("random")
    tv, ti = torch.topk(lp[r], K)
    assert plain["ids"][r].tolist() == ti.tolist() and (plain["vals"][r] - tv).abs().max() < 1e-12
    assert (plain["lse"] - torch.logsumexp(x.double(), -1)).abs().max() < 1e-12
    res = GR.lm_topk(x, V, tc["banned"], tc["flags"], GR.TOPK_SEP, K)
    for r in range(x.shape[0]):
        cv = x[r].tolist()
        f = int(tc["flags"][r])
        for b in tc["banned"].tolist():
            if 0 <= b < V:
                cv[b] = -math.inf
        if f & 1:
            cv[GR.TOPK_SEP] = -math.inf
        if f & 2:
            cv = [c if j == GR.TOPK_SEP else -math.inf for j, c in enumerate(cv)]
        order = sorted(range(V), key=lambda j: (-cv[j], j))[:K]
        assert res["ids"][r].tolist() == order, names[r]
        want = torch.tensor([cv[j] for j in order], dtype=torch.float64) - torch.logsumexp(x[r].double(), -1)
        assert torch.equal(torch.isfinite(res["vals"][r]), torch.isfinite(want)), names[r]
        fin = torch.isfinite(want)
        assert (res["vals"][r][fin] - want[fin]).abs().max() < 1e-9 if fin.any() else True
    assert res["ids"][names.index("everything banned")].tolist() == list(range(K))
    assert not torch.isfinite(res["vals"][names.index("everything banned")]).any()
    assert int(torch.isfinite(res["vals"][names.index("sep forced")]).sum()) == 1


def test_f32_restatements_inside_budget():
    """The recorded constants: the float32 restatements in the kernels' order of operations stay inside the budgets, with the
    factor 8 the constants were chosen with (a subset of the inputs here; `python -m oracle.generate_ref` measures all)."""
    assert GR.C_DEC >= 8 * GR.DEC_MEASURED and GR.C_LSE >= 8 * GR.LSE_MEASURED
    assert math.log2(GR.C_DEC) % 1 == 0 and math.log2(GR.C_LSE) % 1 == 0
    subset = GR.decode_cases()[3::16] + [GR.truncation_case(), GR.probe_case()]
    wd, wl = GR.measure(subset, topk_vs=(16, 257, 1000, 30522))
    print(f"\nworst |fp32 restatement - fp64| / budget term: attn_decode {wd:.3f} (recorded {GR.DEC_MEASURED}, C_DEC {GR.C_DEC}), "
          f"lm_topk lse {wl:.3f} (recorded {GR.LSE_MEASURED}, C_LSE {GR.C_LSE})")
    assert wd <= GR.DEC_MEASURED * 1.001 and wl <= GR.LSE_MEASURED * 1.001
    case = subset[-1]
    args = GR.decode_args(case, GR.decode_views(case))
    ref = GR.attn_decode(*args)
    got = GR.attn_decode_f32(*args).to(BF16).double()                    # the kernel's last step: round to bf16
    assert GR.worst_ratio(got, ref["out"], ref["E"]) <= 1.0


def test_budgets_do_not_loosen():
    """Near 0 the budgets never exceed the existing suite's 1e-4 (lse) and 1e-5 (vals); only the rows offset by +-1e4 are wider,
    and there by about what fp32 can represent."""
    tc = GR.topk_case(30522)
    res = GR.lm_topk(tc["x"], 30522, tc["banned"], tc["flags"], GR.TOPK_SEP, 16)
    far = torch.tensor([n.startswith("offset") for n in tc["names"]])
    assert far.sum() == 2 and (res["lse"].abs()[far] > 9e3).all() and (res["lse"].abs()[~far] < GR.NEAR).all()
    assert (res["E_lse"][~far] <= 1e-4).all() and (res["E_val"][~far] <= 1e-5).all()
    half_ulp = 2.0 ** -11                                                    # of fp32 in [8192, 16384)
    assert (res["E_lse"][far] >= half_ulp).all() and (res["E_lse"][far] <= 16 * half_ulp).all()
    x = torch.randn(24, 30522, generator=torch.Generator().manual_seed(1)) * 3   # the data of test_lm_topk_matches_float64
    res = GR.lm_topk(x, 30522, [0, 101, 103], None, GR.TOPK_SEP, 16)
    assert (res["E_lse"] <= 1e-4).all() and (res["E_val"] <= 1e-5).all()


def test_kv_update_chain_equals_python_lists():
    g = torch.Generator().manual_seed(4)
    layers, slots, pcap, ldp, width, M = 2, 6, 6, 24, 16, 12
    rnd = lambda *shape: torch.randint(-30000, 30000, shape, generator=g, dtype=torch.int16).view(BF16)      # noqa: E731
    bufs = [rnd(layers, slots, pcap, ldp), rnd(layers, slots, pcap, ldp)]
    plen = torch.zeros(slots, dtype=torch.int32)
    hist = [[] for _ in range(slots)]                                        # per hypothesis: list of [layers, width] rows
    cur = 0
    for step in range(5):
        stash = rnd(layers, M, 40)
        parent = [torch.arange(slots), torch.full((slots,), 2), torch.randperm(slots, generator=g),
                  torch.randint(0, slots, (slots,), generator=g), torch.randint(0, slots, (slots,), generator=g)][step]
        new_kv = stash[0][:, 8:]
        before = bufs[1 - cur].clone()
        bufs[1 - cur], plen = GR.kv_cache_update(bufs[cur], bufs[1 - cur], new_kv, parent, plen, layers, slots, pcap, width, M * 40, 2)
        hist = [hist[int(p)] + [stash[:, 2 * int(p), 8:8 + width]] for p in parent]
        cur = 1 - cur
        assert plen.tolist() == [step + 1] * slots
        for s in range(slots):
            got = bufs[cur][:, s, :step + 1, :width].view(torch.int16)
            assert torch.equal(got, torch.stack(hist[s], 1).view(torch.int16)), (step, s)
        keep = torch.ones_like(before, dtype=torch.bool)
        keep[:, :, :step + 1, :width] = False
        assert torch.equal(bufs[cur].view(torch.int16)[keep], before.view(torch.int16)[keep])      # nothing else written


if __name__ == "__main__":
    raise SystemExit(pytest.main([__file__, "-q", "-s"]))
