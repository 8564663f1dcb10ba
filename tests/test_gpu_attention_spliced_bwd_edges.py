"""The training pair of the spliced attention launch (unimm_attn_spliced_fwd / unimm_attn_spliced_bwd) against the fp64
restatement of one launch (oracle/attention_ref.py with `kshared=`, whose autograd sums a shared row's gradient over every
sequence that attends it), with the buffer discipline of tests/test_gpu_attention_edges.py: guard rows, NaN-pattern sentinels
in every output, Q / K / V and their gradients as column slices of wider buffers, mask bits set where they must be ignored,
loud keys on both sides of each splice boundary.

A launch is a list of GROUPS: a shared segment of s rows and members with p private rows each (query rows and key rows).
Shared lengths sit on every 32-key tile edge (and one above 224, where the wave of the private tile also owns a shared tile);
the members of different groups are interleaved in the batch, so no group is contiguous.

Gates are tests/test_gpu_attention_edges.py's GATES, per head and valid row, on the private rows AND on the shared rows: the
shared rows are accumulated in fp32 over the group and rounded once, so their error is that of one sequence's row."""
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import attention_ref as AR
from tests.test_gpu_attention_edges import DEV, GATES, GUARD, LEAD, LOUD, NAN16, NAN32, _nan_like, sentinel_ok

pytestmark = pytest.mark.gpu

D, TQ, TK = 64, 32, 256
# group = (s, [(ql, kl, has_segment), ...]); Case: groups, heads, ks_ins, order, dropout p, accumulate
Case = namedtuple("Case", "name groups H ins order p acc")


def _members(n, ps, seg=True):
    return [(ps[i % len(ps)], ps[(i + 1) % len(ps)] if i % 3 == 2 else ps[i % len(ps)], seg) for i in range(n)]


EDGE_GROUPS = [
    (1, _members(1, [32])), (31, _members(2, [17, 3])), (32, _members(16, [3, 17, 32])), (33, _members(1, [17])),
    (64, _members(2, [32, 3])), (65, _members(1, [3])), (223, _members(2, [32, 17])), (224, _members(2, [32, 3])),   # 224 + 32 = 256
    (250, _members(2, [3, 5])),                                                                                     # a shared tile on the private wave
]
MIXED_GROUPS = [
    (33, [(17, 17, True), (3, 3, False), (32, 32, True)]),           # a member without a segment (ks_len = 0)
    (65, [(5, 9, False)]),                                           # a group whose only member has none: its rows get nothing
    (224, [(32, 32, True)]), (1, _members(2, [3])), (64, _members(16, [17, 3, 32])),
]
CASES = [
    Case("edges ks_ins=1 order p=0.1", EDGE_GROUPS, 2, 1, True, 0.1, False),
    Case("edges ks_ins=0", EDGE_GROUPS, 2, 0, False, 0.0, False),
    Case("mixed ks_ins=1 accumulate", MIXED_GROUPS, 2, 1, False, 0.0, True),
    Case("mixed ks_ins=0 p=0.1 accumulate order", MIXED_GROUPS, 2, 0, True, 0.1, True),
    Case("12 heads ks_ins=1 p=0.1", [(33, _members(2, [17, 3])), (65, _members(3, [3, 32, 17]))], 12, 1, False, 0.1, False),
]


def build(c, seed):
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    H, HD, ins = c.H, c.H * D, c.ins
    # interleave the groups' members: round-robin over the groups
    todo = [list(enumerate(m)) for _, m in c.groups]
    seqs = []                                                        # (group, ql, kl, has_segment)
    while any(todo):
        for gi, t in enumerate(todo):
            if t:
                _, (ql, kl, seg) = t.pop(0)
                seqs.append((gi, ql, kl, seg))
    B, G = len(seqs), len(c.groups)
    gid = np.array([s[0] for s in seqs])
    ql = np.array([s[1] for s in seqs])
    kl = np.array([s[2] for s in seqs])
    seg = np.array([s[3] for s in seqs])
    s_len = np.array([s for s, _ in c.groups])
    q_off = LEAD + np.concatenate([[0], np.cumsum(ql)[:-1]])
    k_off = LEAD + np.concatenate([[0], np.cumsum(kl)[:-1]])
    Rq = LEAD + int(ql.sum()) + GUARD
    s_off = LEAD + int(kl.sum()) + GUARD + np.concatenate([[0], np.cumsum(s_len + 3)[:-1]])      # 3 guard rows between segments
    Rk = int(s_off[-1] + s_len[-1]) + GUARD
    ks_off = s_off[gid]
    ks_len = np.where(seg, s_len[gid], 0)
    nk = kl + ks_len
    assert (nk <= TK).all() and (ql <= TQ).all() and (kl <= 32).all()
    qbuf = torch.randn((Rq, 3 * HD), generator=g).bfloat16()
    kbuf = torch.randn((Rk, 3 * HD), generator=g).bfloat16()
    scale = 1.0 / math.sqrt(D)
    nw = TK // 32
    bits = rng.random((B, TQ, TK)) < 0.6
    bits[:, :, 0] = True
    for b in range(B):
        bits[b, :, nk[b]:] = True                                    # past the keys: set, must be ignored
        bits[b, ql[b]:, :] = True                                    # query rows past q_len: set, must not matter
        if ql[b] >= 3 and b % 2 == 0:
            bits[b, ql[b] - 2, :nk[b]] = False                       # a fully masked row
    for b in range(B):                                               # loud keys
        kr = AR.key_rows(b, k_off, kl, ks_off, ks_len, ins)
        want = [(nk[b] - 1, True), (nk[b] // 2, False)]
        if ks_len[b] > 0:
            want += [(pos, True) for pos in (ins - 1, ins, ins + ks_len[b] - 1, ins + ks_len[b]) if 0 <= pos < nk[b]]
        rows = [qi for qi in list(dict.fromkeys([0, ql[b] - 1, ql[b] // 2] + list(range(1, ql[b])))) if not (ql[b] >= 3 and b % 2 == 0 and qi == ql[b] - 2)]
        for (pos, attend), qi in zip(want, rows):
            bits[b, qi, pos] = attend
            kk = kbuf[kr[pos], HD:2 * HD].float().reshape(H, D)
            cq = LOUD / (scale * (kk * kk).sum(1, keepdim=True))
            qbuf[q_off[b] + qi, :HD] = (cq * kk).reshape(HD).bfloat16()
    words = AR.pack_bits(bits)                                       # [B, TQ, nw]
    order = np.argsort(-(ql + nk), kind="stable").astype(np.int32) if c.order else None
    dout_buf = torch.randn((Rq, HD + 16), generator=g).bfloat16()
    seed_kv = (0.5 * torch.randn((Rk, 2 * HD), generator=g)).bfloat16()     # what the shared rows hold before an accumulating launch
    from unimm_amd import lib
    g_first, g_seq = lib.group_lists(gid, G)
    live = np.array([bool(seg[gid == gi].any()) for gi in range(G)])  # groups some member names
    srows = np.concatenate([np.arange(s_off[gi], s_off[gi] + s_len[gi]) for gi in range(G) if live[gi]] or [np.zeros(0, np.int64)]).astype(np.int64)
    prows = np.concatenate([np.arange(k_off[b], k_off[b] + kl[b]) for b in range(B)]).astype(np.int64)
    qrows = np.concatenate([np.arange(q_off[b], q_off[b] + ql[b]) for b in range(B)]).astype(np.int64)
    return dict(c=c, B=B, G=G, H=H, HD=HD, ql=ql, kl=kl, nk=nk, q_off=q_off, k_off=k_off, ks_off=ks_off, ks_len=ks_len, Rq=Rq, Rk=Rk,
                qbuf=qbuf, kbuf=kbuf, dout_buf=dout_buf, seed_kv=seed_kv, words=words, bits=bits, nw=nw, scale=scale, order=order,
                g_first=g_first, g_seq=g_seq, srows=srows, prows=prows, qrows=qrows)


def _i32(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32, device=DEV)


def _drop(c, seed):
    from unimm_amd import dropout as DR
    return DR.drop_arg(c.p, DR.make_key(11, 3, seed))


def run(s, drop, backward=True, entry="spliced"):
    from unimm_amd import lib
    c, B, H, HD = s["c"], s["B"], s["H"], s["HD"]
    qbuf, kbuf = s["qbuf"].to(DEV), s["kbuf"].to(DEV)
    q, k, v = qbuf[:, :HD], kbuf[:, HD:2 * HD], kbuf[:, 2 * HD:]
    words = torch.from_numpy(s["words"].view(np.int32)).to(DEV)
    obuf = _nan_like(s["Rq"], HD + 24, False)
    lse_buf = torch.full((B * H * TQ + 64,), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    out, lse = obuf[:, 8:8 + HD], lse_buf[:B * H * TQ].view(B, H, TQ)
    order = _i32(s["order"]) if s["order"] is not None else None
    qvar, kvar = (_i32(s["q_off"]), _i32(s["ql"]), None, order), (_i32(s["k_off"]), _i32(s["kl"]))
    kshared = (_i32(s["ks_off"]), _i32(s["ks_len"]), c.ins)
    if entry == "spliced":
        lib.attn_spliced_fwd(q, k, v, out, lse, words, B, H, TQ, TK, D, s["scale"], s["nw"], TQ * s["nw"], drop, qvar, kvar, kshared)
    else:
        lib.attn_fwd(q, k, v, out, lse, words, B, H, TQ, TK, D, s["scale"], s["nw"], TQ * s["nw"], drop, qvar=qvar, kvar=kvar, kshared=kshared)
    res = dict(obuf=obuf, lse_buf=lse_buf)
    if backward:
        dout = s["dout_buf"].to(DEV)[:, 16:16 + HD]
        gq, gk = _nan_like(s["Rq"], HD + 24, False), _nan_like(s["Rk"], 2 * HD + 32, False)
        dq, dk, dv = gq[:, 8:8 + HD], gk[:, 8:8 + HD], gk[:, HD + 24:2 * HD + 24]
        if c.acc:
            sr = torch.from_numpy(s["srows"]).to(DEV)
            sk = s["seed_kv"].to(DEV)
            dk[sr] = sk[sr, :HD]
            dv[sr] = sk[sr, HD:]
        lib.attn_spliced_bwd(q, k, v, out, dout, lse, dq, dk, dv, words, B, H, TQ, TK, D, s["scale"], s["nw"], TQ * s["nw"], drop,
                             qvar, kvar, kshared, (_i32(s["g_first"]), _i32(s["g_seq"])), accumulate=c.acc)
        res.update(gq=gq, gk=gk)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def reference(s, drop, out_arg):
    c, HD = s["c"], s["HD"]
    r = AR.attention(s["qbuf"][:, :HD], s["kbuf"][:, HD:2 * HD], s["kbuf"][:, 2 * HD:], s["words"], B=s["B"], H=s["H"], Tq=TQ, Tk=TK, D=D,
                     scale=s["scale"], mask_q_stride=s["nw"], mask_b_stride=TQ * s["nw"], qvar=(s["q_off"], s["ql"]),
                     kvar=(s["k_off"], s["kl"]), kshared=(s["ks_off"], s["ks_len"], c.ins), drop=drop,
                     dout=s["dout_buf"][:, 16:16 + HD], out_arg=out_arg)
    if c.acc:                                                        # the rows held these values: they are part of the one rounding
        sr = torch.from_numpy(s["srows"])
        sk = s["seed_kv"].double()
        for key, cols in (("dk", slice(0, HD)), ("dv", slice(HD, 2 * HD))):
            for suf in ("", "_bwd"):
                r[key + suf] = r[key + suf].clone()
                r[key + suf][sr] += sk[sr, cols]
    return r


def row_errors(got, ref, rows, H):
    """tests/test_gpu_attention_edges.py's row_errors for H heads: max over valid rows and heads of max|got - ref| over the head's
    columns / max(row max|ref|, 2^-3 head max|ref|)"""
    g = got[rows].double().reshape(len(rows), H, D)
    r = ref[rows].double().reshape(len(rows), H, D)
    assert torch.isfinite(g).all(), "non-finite values in valid rows"
    rowmax = r.abs().amax(-1)
    floor = 2.0 ** -3 * rowmax.amax(0, keepdim=True)
    e = (g - r).abs().amax(-1) / torch.maximum(rowmax, floor).clamp_min(1e-30)
    return float(e.max())


def check(s, got, ref):
    c, B, H, HD = s["c"], s["B"], s["H"], s["HD"]
    qrows, krows = s["qrows"], np.concatenate([s["prows"], s["srows"]])
    errs = {"out": row_errors(got["obuf"][:, 8:8 + HD], ref["out"], qrows, H)}
    n, where = sentinel_ok(got["obuf"], qrows, 8, 8 + HD, NAN16)
    assert n == 0, f"out: {n} elements outside the valid rows / head columns were written, e.g. {where}"
    lse = got["lse_buf"][:B * H * TQ].view(B, H, TQ).double()
    lbits = got["lse_buf"].view(torch.int32)
    past = torch.ones((B, H, TQ), dtype=torch.bool)
    live = torch.zeros((B, H, TQ), dtype=torch.bool)
    for b in range(B):
        past[b, :, :s["ql"][b]] = False
        live[b, :, :s["ql"][b]] = torch.from_numpy(s["bits"][b, :s["ql"][b], :s["nk"][b]].any(-1))[None]
    assert bool((lbits[:B * H * TQ].view(B, H, TQ)[past] == NAN32).all()), "lse written past q_len"
    assert bool((lbits[B * H * TQ:] == NAN32).all()), "lse written past [B, H, Tq]"
    d = (lse - ref["lse"]).abs()
    errs["lse"] = float(d[live].max())
    dead = ~live & ~past
    if dead.any():
        errs["lse_dead"] = float(d[dead].max())
    if "gq" in got:
        gk = got["gk"]
        for k, g, rows in (("dq", got["gq"][:, 8:8 + HD], qrows), ("dk", gk[:, 8:8 + HD], krows), ("dv", gk[:, HD + 24:2 * HD + 24], krows)):
            errs[k] = row_errors(g, ref[k + "_bwd"], rows, H)
            errs[k + "_exact"] = float((g[rows].double() - ref[k][rows]).abs().max() / ref[k][rows].abs().max())
        if len(s["srows"]):                                          # the shared rows on their own: no wider gate
            errs["dk_shared"] = row_errors(gk[:, 8:8 + HD], ref["dk_bwd"], s["srows"], H)
            errs["dv_shared"] = row_errors(gk[:, HD + 24:2 * HD + 24], ref["dv_bwd"], s["srows"], H)
        n, where = sentinel_ok(got["gq"], qrows, 8, 8 + HD, NAN16)
        assert n == 0, f"dq: {n} elements outside the valid rows / head columns were written, e.g. {where}"
        gkb = gk.view(torch.int16)
        keep = torch.ones(gkb.shape, dtype=torch.bool)
        kr = torch.as_tensor(krows, dtype=torch.long)[:, None]
        keep[kr, torch.arange(8, 8 + HD)[None, :]] = False
        keep[kr, torch.arange(HD + 24, 2 * HD + 24)[None, :]] = False
        bad = (gkb != NAN16) & keep
        assert not bad.any(), f"dk / dv: {int(bad.sum())} elements outside the valid rows / head columns were written, e.g. {bad.nonzero()[:4].tolist()}"
    print(f"\n{c.name}: " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(errs.items())))
    gates = dict(GATES, dk_shared=GATES["dk"], dv_shared=GATES["dv"])
    for k, v in errs.items():
        assert v <= gates[k], (c.name, k, v, errs)
    return errs


def _same(a, b):
    for k in a:
        if not torch.equal(a[k].view(torch.int16 if a[k].dtype == torch.bfloat16 else torch.int32),
                           b[k].view(torch.int16 if b[k].dtype == torch.bfloat16 else torch.int32)):
            return k
    return None


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_spliced_pair_against_fp64(c):
    seed = sum(map(ord, c.name))
    s = build(c, seed)
    drop = _drop(c, seed)
    got = run(s, drop)
    ref = reference(s, drop, got["obuf"][:, 8:8 + s["HD"]])
    check(s, got, ref)
    again = run(s, drop)
    assert _same(got, again) is None, f"two identical launches differ in {_same(got, again)}"


def test_spliced_fwd_equals_attn_fwd_without_dropout():
    c = CASES[1]
    s = build(c, 5)
    a, b = run(s, (0, 0, 1.0), backward=False), run(s, (0, 0, 1.0), backward=False, entry="plain")
    assert _same(a, b) is None, f"unimm_attn_spliced_fwd and unimm_attn_fwd differ in {_same(a, b)}"


def test_refusals_write_nothing():
    from unimm_amd import lib
    H, HD = 2, 2 * D
    B = 2
    qkv = torch.randn((80, 3 * HD + 8), device=DEV).bfloat16()
    q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:3 * HD]
    dout = torch.randn((80, HD), device=DEV).bfloat16()
    words = torch.full((B, TQ, 8), -1, dtype=torch.int32, device=DEV)
    qv, kv = (_i32([0, 40]), _i32([3, 4])), (_i32([0, 40]), _i32([3, 4]))
    ks, gr = (_i32([8, 48]), _i32([20, 20]), 1), (_i32([0, 1, 2]), _i32([0, 1]))
    bufs = {}

    def fresh():
        bufs.update(out=_nan_like(80, HD, False), gq=_nan_like(80, HD, False), gk=_nan_like(80, HD, False), gv=_nan_like(80, HD, False),
                    lse=torch.full((B, H, TQ), NAN32, dtype=torch.int32, device=DEV).view(torch.float32))
        return bufs

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32) == (NAN16 if t.dtype == torch.bfloat16 else NAN32)).all())
                   for t in bufs.values())

    def fwd(code, q=q, lse=True, Tq=TQ, Tk=TK, Dh=D, qv=qv, kv=kv, ks=ks):
        b = fresh()
        with pytest.raises(lib.UnimmHipError, match=code):
            lib.attn_spliced_fwd(q, k, v, b["out"], b["lse"] if lse else None, words, B, H, Tq, Tk, Dh, 0.125, 8, TQ * 8, (0, 0, 1.0), qv, kv, ks)
        assert untouched(), code

    def bwd(code, q=q, Tq=TQ, Tk=TK, Dh=D, kv=kv, ks=ks, gr=gr, dk=None):
        b = fresh()
        lse = torch.zeros((B, H, TQ), device=DEV)
        with pytest.raises(lib.UnimmHipError, match=code):
            lib.attn_spliced_bwd(q, k, v, dout, dout, lse, b["gq"], b["gk"] if dk is None else dk, b["gv"], words, B, H, Tq, Tk, Dh, 0.125, 8,
                                 TQ * 8, (0, 0, 1.0), qv, kv, ks, gr)
        assert untouched(), code

    none2 = (None, None)
    for f in (fwd, bwd):
        f("UNIMM_E_ARG", Dh=128)
        f("UNIMM_E_ARG", Tq=33)                                      # more than 32 private rows
        f("UNIMM_E_ARG", Tk=257)
        f("UNIMM_E_ARG", ks=(ks[0], ks[1], -1))
        f("UNIMM_E_ARG", ks=(None, None, 1))
        f("UNIMM_E_ARG", kv=None)
        f("UNIMM_E_ALIGN", q=qkv[:, 4:4 + HD])                       # 8-byte aligned base
    fwd("UNIMM_E_ARG", lse=False)
    fwd("UNIMM_E_ARG", qv=None)
    bwd("UNIMM_E_ARG", gr=none2)
    bwd("UNIMM_E_ARG", gr=(_i32([0]), gr[1]))                        # no group
    bwd("UNIMM_E_ALIGN", dk=_nan_like(80, HD + 4, False)[:, :HD])    # row stride not a multiple of 8
    # unimm_attn_fwd keeps its own refusal of a segment with dropout
    b = fresh()
    with pytest.raises(lib.UnimmHipError, match="UNIMM_E_ARG"):
        lib.attn_fwd(q, k, v, b["out"], b["lse"], words, B, H, TQ, TK, D, 0.125, 8, TQ * 8, (1, 1 << 28, 1.1), qvar=qv, kvar=kv, kshared=ks)
    assert untouched()


def test_segment_rows_sum_against_fp64():
    """unimm_segment_rows_sum_bf16: the region gradients of a group's text blocks, added in fp32 in list order and rounded once:
    |got - fp64 sum| <= 2^-8 |sum| + 2^-8 2^-7 sum |terms| (one bf16 rounding, half an ulp = 2^-9 relative, plus the fp32
    accumulation of at most 16 terms, far below it); nothing outside the G blocks x W columns changes; a second launch repeats the bits."""
    from unimm_amd import lib
    R, W, n_items = 37, 264, 23                                      # W: 33 16-byte chunks, more than one per thread wave
    g = torch.Generator().manual_seed(4)
    gid = np.array([3, 0, 2, 0, 2, 2, 0, 2] + [2] * 12 + [0, 3, 2])  # groups of 4, 0, 16 and 2 items (+ group 1: none), interleaved
    first, items = lib.group_lists(gid, 4)
    assert sorted(np.diff(first).tolist()) == [0, 2, 4, 17]
    src = torch.randn((n_items * R, W + 16), generator=g).bfloat16()
    dbuf = _nan_like(4 * R + GUARD, W + 24, False)
    for rep in range(2):
        d2 = _nan_like(4 * R + GUARD, W + 24, False)
        lib.segment_rows_sum_bf16(src.to(DEV)[:, 8:8 + W], _i32(first), _i32(items), d2[:, 16:16 + W], R, W)
        torch.cuda.synchronize()
        if rep == 0:
            dbuf = d2
        else:
            assert torch.equal(dbuf.view(torch.int16), d2.view(torch.int16)), "two identical launches differ"
    blocks = src[:, 8:8 + W].double().view(n_items, R, W)
    ref = torch.stack([blocks[gid == gi].sum(0) for gi in range(4)])                       # [4, R, W]; an empty group sums to zero
    mag = torch.stack([blocks[gid == gi].abs().sum(0) for gi in range(4)])
    got = dbuf.cpu()[:4 * R, 16:16 + W].double().view(4, R, W)
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    assert bool((err <= 2.0 ** -8 * ref.abs() + 2.0 ** -15 * mag).all()), float(err.max())
    n, where = sentinel_ok(dbuf.cpu(), np.arange(4 * R), 16, 16 + W, NAN16)
    assert n == 0, where
    for bad in (dict(W=W + 4), dict(R=0)):
        with pytest.raises(lib.UnimmHipError, match="UNIMM_E_A"):
            lib.segment_rows_sum_bf16(src.to(DEV)[:, 8:8 + W], _i32(first), _i32(items), dbuf[:, 16:16 + W], bad.get("R", R), bad.get("W", W))


def test_ordered_embedding_backward_against_fp64_and_the_atomic_kernel():
    """unimm_embed_bwd_rows + unimm_rows_scatter_sum_f32 (the shared step's embedding gradient, no atomics):
    the scatter against an fp64 index_add (fp32 sums of at most 40 addends: |err| <= 40 * 2^-24 * sum |addends|), skipped keys
    (negative, past the table) and rows outside the keys untouched, two launches bit-identical; and the pair against
    unimm_embed_bwd on the same inputs (the same addends in another order: the same bound with both orders' roundings)."""
    from unimm_amd import lib
    g = torch.Generator().manual_seed(9)
    M, H, V, P = 150, 136, 50, 64                                   # H: not a multiple of 64 or 256
    src = torch.randn((M, H), generator=g).to(DEV)
    key = torch.randint(-1, 7, (M,), generator=g).to(torch.int32)      # runs of ~20 rows per key, some skipped (-1)
    key[::13] = V + 3                                                # past the table: skipped
    ks, order = torch.sort(key.to(DEV), stable=True)
    base = torch.randn((V, H), generator=g).to(DEV)
    outs = []
    for _ in range(2):
        dst = base.clone()
        lib.rows_scatter_sum_f32(src, ks.contiguous(), order.to(torch.int32), dst)
        torch.cuda.synchronize()
        outs.append(dst.cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    ok = (key >= 0) & (key < V)
    ref = base.cpu().double().index_add(0, key[ok].long(), src.cpu().double()[ok])
    mag = base.cpu().double().abs().index_add(0, key[ok].long(), src.cpu().double()[ok].abs())
    assert bool(((outs[0].double() - ref).abs() <= 40 * 2.0 ** -24 * mag).all())
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[key[ok].long()] = False
    assert torch.equal(outs[0][untouched].view(torch.int32), base.cpu()[untouched].view(torch.int32))
    # the pair against the atomic kernel
    ids = torch.randint(0, 9, (M,), generator=g).to(torch.int32).to(DEV)
    pos = torch.randint(0, P, (M,), generator=g).to(torch.int32).to(DEV)
    typ = torch.randint(0, 5, (M,), generator=g).to(torch.int32).to(DEV)
    rows = torch.randperm(M, generator=g).to(DEV)
    tab = lambda n: torch.randn((n, H), generator=g).to(DEV)
    word, post, type_, ext, gamma, beta = tab(V), tab(P), tab(2), tab(10), tab(1).reshape(-1), tab(1).reshape(-1)
    dy = torch.randn((M, H), generator=g).bfloat16().to(DEV)
    drop = _drop(SimpleNamespace(p=0.1), 4)
    Z = lambda n: torch.zeros((n, H), device=DEV)
    part = torch.zeros(lib.colpartials_bytes(H) // 4, device=DEV)
    a = dict(word=Z(V), pos=Z(P), type=Z(2), ext=Z(10), gamma=Z(1).reshape(-1), beta=Z(1).reshape(-1))
    lib.embed_bwd(ids, pos, typ, word, post, type_, ext, gamma, beta, dy, a["word"], a["pos"], a["type"], a["ext"], a["gamma"], a["beta"],
                  part, M, H, drop=drop, rows=rows)
    b = dict(word=Z(V), pos=Z(P), type=Z(2), ext=Z(10), gamma=Z(1).reshape(-1), beta=Z(1).reshape(-1))
    drow = torch.empty((M, H), device=DEV)
    lib.embed_bwd_rows(ids, pos, typ, word, post, type_, ext, gamma, beta, dy, drow, b["type"], b["gamma"], b["beta"], part, M, H,
                       drop=drop, rows=rows)
    tt = typ[rows]
    for k_, name in ((ids[rows], "word"), (pos[rows], "pos"), (torch.where(tt >= 2, tt - 2, torch.full_like(tt, -1)), "ext")):
        ks, order = torch.sort(k_, stable=True)
        lib.rows_scatter_sum_f32(drow, ks.contiguous(), order.to(torch.int32), b[name])
    torch.cuda.synchronize()
    for name in a:
        x, y = a[name].double().cpu(), b[name].double().cpu()
        assert torch.isfinite(y).all() and float(x.abs().max()) > 0, name
        assert float((x - y).abs().max()) <= 2 * M * 2.0 ** -24 * float(drow.abs().max()) * 8, (name, float((x - y).abs().max()))
