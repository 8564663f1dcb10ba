"""unimm_attn_verify and unimm_kv_cache_append per element at every edge, against tests/spec_ref.py (fp64 restatements built on
oracle/generate_ref.py; the budget and its measured constant are derived there).  The conventions are those of
tests/test_gpu_generate_edges.py: guard rows around every buffer, a row stride wider than the payload, outputs pre-filled with a
sentinel that everything outside the written region must keep, NaN in every input element the contract says is not read."""
import pytest
import torch

from oracle import generate_ref as GR
from tests import spec_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
GUARD = GR.GUARD
SENT = -768.0
DEV = "cuda"


def launch(case, fn):
    """One launch of `fn` (lib.attn_verify or lib.attn_decode) on device copies of the case's buffers -> out [R, H D]
    float64; checks that nothing else was written."""
    HD, R = case["H"] * 64, case["R"]
    new, ctx = case["new"].to(DEV), case["ctx"].to(DEV)
    priv = case["priv"].to(DEV) if case["priv"] is not None else None
    outbuf = torch.full((GUARD + R + GUARD, HD + 8), SENT, dtype=BF16, device=DEV)
    out = outbuf[GUARD:GUARD + R, :HD]
    q, k, v, ck, cv, pk, pv = GR.decode_views(case, new, ctx, priv)
    i32 = lambda t: t.to(DEV, torch.int32)      # noqa: E731
    fn(q, k, v, out, ck, cv, i32(case["ctx_off"]), i32(case["ctx_len"]), pk, pv, i32(case["plen"]), case["G"], case["beams"],
       case["nr"], case["H"], case["pcap"], case["scale"])
    torch.cuda.synchronize()
    ob = outbuf.cpu().float()
    outside = torch.ones_like(ob, dtype=torch.bool)
    outside[GUARD:GUARD + R, :HD] = False
    assert (ob[outside] == SENT).all(), "wrote outside out[:, :H * 64]"
    return ob[GUARD:GUARD + R, :HD].double()


def check_verify(case, what):
    from unimm_amd.lib import attn_verify
    got = launch(case, attn_verify)
    ref = SR.attn_verify(*GR.decode_args(case, GR.decode_views(case)))
    assert torch.isfinite(ref["out"]).all()
    assert torch.isfinite(got).all(), (what, "a NaN: an input outside the key set was read")
    bad = (got - ref["out"]).abs() > ref["E"]
    if bad.any():
        r, col = [int(x) for x in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the budget, first (row {r}, col {col}, {int(ref['nk'][r])} keys): "
                             f"got {got[r, col]:.6f} want {ref['out'][r, col]:.6f} E {ref['E'][r, col]:.2e}")
    return GR.worst_ratio(got, ref["out"], ref["E"]), ref, got


@pytest.mark.parametrize("beams,nr", SR.VER_BN)
@pytest.mark.parametrize("H", SR.VER_H)
def test_attn_verify_edges(H, beams, nr):
    """G in {1, 3} with the contexts in reverse group order; ctx_len from {0, 1, 63, 64, 65, 255, 256}; plen from {0, 1, 3, pcap,
    pcap + 2 (clamped), -1 (clamped)}; private rows at and past the clamped plen are NaN."""
    worst = 0.0
    for case in SR.verify_cross_cases(H, beams, nr):
        what = f"H {H} beams {beams} nr {nr} G {case['G']} pcap {case['pcap']} ctx_len {case['ctx_len'].tolist()}"
        worst = max(worst, check_verify(case, what)[0])
    print(f"\nattn_verify edges H = {H}, beams = {beams}, nr = {nr}: worst |err| / E = {worst:.3f}")


def test_attn_verify_truncation_and_clamps():
    """ctx_len = 256, nr = 32: 32 private rows whatever plen and pcap say (rows 32 .. are NaN here); plen > pcap behaves as pcap
    and a negative plen as 0, to the bit."""
    w, ref, _ = check_verify(SR.truncation_case(), "ctx 256, nr 32, pcap 40")
    assert ref["nk"].tolist() == [256 + 32 + i // 2 + 1 + i % 2 for i in range(32)] * 3
    a = GR.decode_case(3, 3, 2, 6, 1, 5, [65], [9, -3])
    b = dict(a, plen=torch.tensor([5, 0], dtype=torch.int32))
    wa, _, ga = check_verify(a, "plen [9, -3] of pcap 5")
    wb, _, gb = check_verify(b, "plen [5, 0] of pcap 5")
    assert torch.equal(ga, gb)
    z = GR.decode_case(4, 2, 1, 4, 2, 0, [0, 7], [0, -1])                  # pcap = 0: NULL private pointers; ctx_len 0
    wz = check_verify(z, "pcap 0")[0]
    print(f"\nattn_verify clamps: worst |err| / E = {max(w, wa, wb, wz):.3f}")


def test_attn_verify_key_set_probes():
    """Each probing row puts its mass on one chosen key; another copy row, a later pair's answer row or the next slot's rows would
    take all of it if they were seen (spec_ref.probe_case)."""
    case = SR.probe_case()
    w, ref, got = check_verify(case, "probes")
    for qrow, h, vid in case["probes"]:
        lo, hi = float(got[qrow, h * 64]), float(got[qrow, h * 64 + 1])
        assert (round(lo), round(hi)) == (vid % 64, vid // 64), (qrow, h, vid, lo, hi)
    print(f"\nattn_verify probes ({len(case['probes'])}): worst |err| / E = {w:.3f}")


@pytest.mark.parametrize("H,G,beams", [(1, 1, 1), (3, 3, 16), (12, 2, 5)])
def test_attn_verify_nr2_is_attn_decode_bit_for_bit(H, G, beams):
    from unimm_amd import lib as L
    from unimm_amd.lib import attn_verify
    pls = (0, 1, 3, 4, 5, 20, 22, -1)
    case = GR.decode_case(600 + H, H, beams, 2, G, 20, [(9, 256, 64)[g % 3] for g in range(G)],
                          [pls[s % len(pls)] for s in range(G * beams)])
    assert torch.equal(launch(case, attn_verify), launch(case, L.attn_decode))


def test_attn_verify_refusals():
    from unimm_amd import lib as L
    from unimm_amd.lib import attn_verify
    for beams, nr in ((1, 3), (1, 1), (1, 34), (2, 18), (17, 2), (1, 0)):
        case = GR.decode_case(1, 1, 1, 2, 1, 4, [5], [0])
        case.update(beams=beams, nr=nr)
        with pytest.raises(L.UnimmHipError, match="UNIMM_E_SHAPE"):
            launch(case, attn_verify)


# ---------------------------------------------------------------------------------------------------------------------------
# unimm_kv_cache_append
# ---------------------------------------------------------------------------------------------------------------------------
def append_case(layers, slots, pcap, max_count, count, plen, seed, step=2):
    g_ = torch.Generator().manual_seed(seed)
    width, ldp = 128, 128 + 8
    mul = step * max(max_count, 1)
    M = slots * mul
    cache = torch.full((layers, slots, pcap, ldp), float("nan"), dtype=BF16)
    stash = torch.full((layers, M, width + 72), float("nan"), dtype=BF16)
    for s in range(slots):
        for j in range(max_count):                                          # only the rows a launch may read are numbers
            stash[:, s * mul + j * step, 64:64 + width] = torch.randn(layers, width, generator=g_).to(BF16)
    return dict(cache=cache, stash=stash, count=torch.tensor(count, dtype=torch.int32), plen=torch.tensor(plen, dtype=torch.int32),
                layers=layers, slots=slots, pcap=pcap, width=width, max_count=max_count, nls=M * (width + 72), mul=mul, step=step)


def run_append(c):
    from unimm_amd.lib import kv_cache_append
    cache, stash = c["cache"].to(DEV), c["stash"].to(DEV)
    po = torch.full((c["slots"] + 2,), -7, dtype=torch.int32, device=DEV)
    kv_cache_append(cache, stash[0][:, 64:], c["count"].to(DEV), c["plen"].to(DEV), po[1:-1], c["layers"], c["slots"], c["pcap"],
                    c["width"], c["max_count"], c["nls"], c["mul"], c["step"])
    torch.cuda.synchronize()
    want, wpo = SR.kv_cache_append(c["cache"], c["stash"][0][:, 64:], c["count"], c["plen"], c["layers"], c["slots"], c["pcap"],
                                   c["width"], c["max_count"], c["nls"], c["mul"], c["step"])
    assert torch.equal(cache.cpu().view(torch.int16), want.view(torch.int16)), "cache rows differ (or a row / column outside was written)"
    assert po.cpu().tolist() == [-7] + wpo.tolist() + [-7]
    return want, wpo


@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("slots", [1, 5])
def test_kv_cache_append_bit_exact(layers, slots):
    """counts 0 .. max_count mixed in one launch; plen at 0 and pcap - 1; every clamp: count > max_count, count < 0, count past
    the capacity, plen > pcap, plen < 0.  The cache starts as NaN everywhere: a row or a column past `width` that must stay is
    still NaN bit for bit, and the NaN rows / columns of the stash were not read (the written rows are all numbers)."""
    pcap, mc = 9, 4
    counts = [3, 0, 4, 9, -2][:slots]
    plens = [0, pcap - 1, 2, 7, 11][:slots] if slots > 1 else [pcap - 1]
    want, wpo = run_append(append_case(layers, slots, pcap, mc, counts, plens, seed=layers * 10 + slots))
    for s in range(slots):
        pl = min(max(plens[s], 0), pcap)
        n = int(wpo[s]) - pl
        assert torch.isfinite(want[:, s, pl:pl + n, :128].float()).all()
    run_append(append_case(layers, slots, pcap, mc, [1, 4, 2, 1, 4][:slots], [-3, 0, 8, 9, 6][:slots], seed=77))
    run_append(append_case(layers, slots, pcap, 1, [1] * slots, [0, 3, 8, 9, 20][:slots], seed=78, step=1))


def test_kv_cache_append_error_codes():
    from unimm_amd import lib as L
    from unimm_amd.lib import kv_cache_append
    layers, slots, pcap, width = 2, 3, 4, 64
    cache = torch.full((layers, slots, pcap, width + 8), SENT, dtype=BF16, device=DEV)
    stash = torch.zeros((layers, slots * 4, width + 8), dtype=BF16, device=DEV)
    cnt = torch.ones(slots, dtype=torch.int32, device=DEV)
    plen = torch.zeros(slots, dtype=torch.int32, device=DEV)
    po = torch.full((slots,), -7, dtype=torch.int32, device=DEV)
    nls = slots * 4 * (width + 8)
    call = lambda nk, pl, pout, w: kv_cache_append(cache, nk, cnt, pl, pout, layers, slots, pcap, w, 2, nls, 4, 2)   # noqa: E731
    with pytest.raises(L.UnimmHipError, match="UNIMM_E_ARG"):
        call(stash[0], plen, plen, width)
    with pytest.raises(L.UnimmHipError, match="UNIMM_E_ALIGN"):
        call(stash[0][:, 4:], plen, po, width)
    with pytest.raises(L.UnimmHipError, match="UNIMM_E_ALIGN"):
        call(stash[0], plen, po, 12)
    with pytest.raises(L.UnimmHipError, match="UNIMM_E_SHAPE"):
        call(stash[0], plen, po, width + 16)
    torch.cuda.synchronize()
    assert (cache.float() == SENT).all() and (po == -7).all()


def test_append_then_verify_chain():
    """The two kernels the way speculative.py uses them: three rounds of attn_verify on every layer's new rows, then one
    kv_cache_append of a varying number of each slot's answer rows (ping-pong plen); the restatement keeps the cache on the host."""
    from unimm_amd.lib import attn_verify, kv_cache_append
    g_ = torch.Generator().manual_seed(31)
    layers, G, nr, pcap, H = 2, 3, 8, 9, 2
    HD, P = H * 64, nr // 2
    M = G * nr
    clen, coff = [9, 17, 64], [70, 2, 100]
    ctx = [GR._poisoned(170, 3 * HD) for _ in range(layers)]
    for c in ctx:
        for g in range(G):
            c[coff[g]:coff[g] + clen[g], HD:] = (torch.randn(clen[g], 2 * HD, generator=g_) * 1.5).to(BF16)
    cache = torch.full((layers, G, pcap, 2 * HD), float("nan"), dtype=BF16)
    cache_d = cache.to(DEV)
    plen = torch.zeros(G, dtype=torch.int32)
    plen_d = [plen.to(DEV), torch.zeros(G, dtype=torch.int32, device=DEV)]
    cur, worst = 0, 0.0
    i32 = lambda t: torch.tensor(t, dtype=torch.int32)              # noqa: E731
    for rnd, counts in enumerate(([4, 1, 2], [0, 3, 4], [2, 4, 4])):   # the last round runs slot 2 into the capacity (6 + 4 > 9)
        stash = (torch.randn(layers, M, 3 * HD, generator=g_) * 1.5).to(BF16)
        stash_d = stash.to(DEV)
        for l in range(layers):
            out = torch.full((M, HD), SENT, dtype=BF16, device=DEV)
            cd, pd = ctx[l].to(DEV), cache_d[l].view(G * pcap, 2 * HD)
            attn_verify(stash_d[l][:, :HD], stash_d[l][:, HD:2 * HD], stash_d[l][:, 2 * HD:], out, cd[:, HD:2 * HD], cd[:, 2 * HD:],
                        i32(coff).to(DEV), i32(clen).to(DEV), pd[:, :HD], pd[:, HD:], plen_d[cur], G, 1, nr, H, pcap, 0.125)
            ph = cache[l].view(G * pcap, 2 * HD)
            ref = SR.attn_verify(stash[l][:, :HD], stash[l][:, HD:2 * HD], stash[l][:, 2 * HD:], ctx[l][:, HD:2 * HD], ctx[l][:, 2 * HD:],
                                 i32(coff), i32(clen), ph[:, :HD], ph[:, HD:], plen, G, 1, nr, H, pcap, 0.125)
            got = out.cpu().double()
            assert torch.isfinite(got).all(), (rnd, l)
            assert ((got - ref["out"]).abs() <= ref["E"]).all(), (rnd, l)
            worst = max(worst, GR.worst_ratio(got, ref["out"], ref["E"]))
        kv_cache_append(cache_d, stash_d[0][:, HD:], i32(counts).to(DEV), plen_d[cur], plen_d[1 - cur], layers, G, pcap, 2 * HD, P,
                        M * 3 * HD, nr, 2)
        cache, plen = SR.kv_cache_append(cache, stash[0][:, HD:], counts, plen, layers, G, pcap, 2 * HD, P, M * 3 * HD, nr, 2)
        cur = 1 - cur
        torch.cuda.synchronize()
        assert torch.equal(cache_d.cpu().view(torch.int16), cache.view(torch.int16)) and plen_d[cur].cpu().tolist() == plen.tolist()
    assert plen.tolist() == [6, 8, 9]
    print(f"\nappend -> verify chain: worst |err| / E = {worst:.3f}")
